"""Measured error of the fused photometric loss (csrc/photo_loss.hip) against the float64
reference, next to the error of the formulation it replaces (fp32 `train_loop.view_loss`,
torch on the same GPU) against the same float64 truth, on every case of
tests/test_photo_loss.py: the golden vectors (the reference's own l1_loss / ssim in float64),
the seeded shapes, the ssim-only and l1-only parts, and one view through the rasterizer.
Metrics as the test: |loss - ref| for l1, ssim and the combined loss; the gradient by
max|grad - ref| / max|ref|.  LOSS_ATOL and GRAD_RTOL of the test are twice the worst fused
figures; the summary lists the cases where a fused figure is above twice torch's.
Usage: python tools/photo_loss_err.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_photo_loss as T  # noqa: E402
from langsplatv2_amd.train_loop import view_loss  # noqa: E402

DEV = torch.device("cuda:0")


def torch_fp32(x, y, lam):
    xt = torch.from_numpy(np.asarray(x)).to(DEV).requires_grad_(True)
    loss = view_loss(xt, torch.from_numpy(np.asarray(y)).to(DEV), lam)
    loss.backward()
    return loss.item(), xt.grad.cpu().numpy()


def record(x, y, ref, lam=T.LAMBDA):
    """ref = (l1, ssim, loss, grad) in float64 for this lam."""
    got = T.gpu_loss(x, y, lam=lam)
    tl, tg = torch_fp32(x, y, lam)
    # the losses leave the GPU as fp32: half an ulp of the value is the floor of either error
    return dict(loss_ref=float(ref[2]), loss_fp32_half_ulp=float(np.spacing(np.float32(ref[2]))) / 2,
                fused=dict(l1_abs=abs(got[0] - float(ref[0])), ssim_abs=abs(got[1] - float(ref[1])),
                           loss_abs=abs(got[2] - float(ref[2])), grad_rel=T.grad_err(got[3], ref[3])),
                torch_fp32=dict(loss_abs=abs(tl - float(ref[2])), grad_rel=T.grad_err(tg, ref[3])))


def main():
    out = {}
    for name in T.GOLD_NAMES:
        z = T._gold(name)
        out["golden_" + name] = record(z["x"], z["y"], (z["l1"], z["ssim"], z["loss"], z["grad"]))
    for shape in T.RANDOM_SHAPES:
        c = T.random_case(shape)
        out["random_" + "x".join(map(str, shape))] = record(c[0], c[1], c[2:])
    c = T.random_case((3, 47, 130))
    out["ssim_only_3x47x130"] = record(c[0], c[1], T.ref64(c[0], c[1], lam=1.0), lam=1.0)
    out["l1_only_3x47x130"] = record(c[0], c[1], T.ref64(c[0], c[1], lam=0.0), lam=0.0)
    _, _, img, gt = T.rendered_case()
    out["render_3x64x96"] = record(img, gt, T.ref64(img, gt))
    worst_loss = max(max(v["fused"][k] for k in ("l1_abs", "ssim_abs", "loss_abs")) for v in out.values())
    worst_grad = max(v["fused"]["grad_rel"] for v in out.values())
    worse = [k for k, v in out.items() if v["fused"]["loss_abs"] > 2 * v["torch_fp32"]["loss_abs"]
             or v["fused"]["grad_rel"] > 2 * v["torch_fp32"]["grad_rel"]]
    out["summary"] = dict(worst_fused_loss_abs=worst_loss, worst_fused_grad_rel=worst_grad,
                          LOSS_ATOL=2 * worst_loss, GRAD_RTOL=2 * worst_grad,
                          cases_where_fused_exceeds_2x_torch=worse)
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
