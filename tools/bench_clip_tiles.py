"""The CLIP input tiles of the kept SAM masks (langsplatv2_amd.clip_tiles,
csrc/clip_tiles.hip) at N = 128 and 384 masks, 1280 x 800 and 1920 x 1080, on
rectangle scenes from the mask-NMS fixture generator
(tests/golden/make_ref_mask_nms.py) with a seeded random frame; every mask gets
a 224 x 224 tile.

  python tools/bench_clip_tiles.py [--iters 200] [--out profiles/clip_tiles_bench.json] [--hip-only]

(--hip-only leaves the two baselines out: the form to run under a kernel trace.)

Per shape, one JSON line per variant (ms, best of 3 alternating rounds, host clock
around work that ends in a device synchronise):
  hip            mask_boxes; clip_tiles in each output form ("u8", "unit", "clip")
                 with the scene's boxes; end to end from packed masks (mask_boxes,
                 then "clip" tiles from those boxes).  Floors: the words the box
                 kernel reads (N x ceil(H W / 64) x 8 B) and the bytes the tile
                 kernel writes (n x 224 x 224 x 3 x element size), as achieved
                 bytes/s and as the ratio of the time to those bytes at PEAK_BPS
  torch          baseline (a), what a user would write on the same GPU, per mask:
                 torch.where over the frame, crop, pad, F.interpolate(bilinear,
                 align_corners=False), then / 255, normalise, half.  NOT bit-equal
                 to the hip path (float bilinear, no 11-bit coefficients); the
                 largest difference of the 0 .. 255 tiles is reported
  host_steps     baseline (b), the reference's host steps per mask restated in
                 numpy: frame copy, masked write, crop, pad; then the stack's
                 float conversion, / 255 and the upload.  cv2.resize is LEFT OUT
                 (cv2 is not a dependency), so this is a lower bound on the
                 reference's time, measured once
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CT = importlib.import_module("langsplatv2_amd.clip_tiles")  # noqa: E402
MN = importlib.import_module("langsplatv2_amd.mask_nms")  # noqa: E402

SHAPES = [(128, 800, 1280), (384, 800, 1280), (128, 1080, 1920), (384, 1080, 1920)]
S = 224
PEAK_BPS = 6.29e12   # the streaming copy rate measured on one MI355X (8.0 TB/s on the data sheet)
ELEM = {"u8": 1, "unit": 4, "clip": 2}


def maker():
    spec = importlib.util.spec_from_file_location("make_ref_mask_nms",
                                                  os.path.join(ROOT, "tests", "golden", "make_ref_mask_nms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scene(N, H, W, dev, seed=0):
    """The generator's boxes rasterised on the device: (N, H, W) bool masks, (N, 4) int32 x, y, w, h boxes
    (tight, as SAM's), and a seeded random (H, W, 3) uint8 frame."""
    rects, _ = maker().rect_boxes(N, H, W, seed)   # y0, y1, x0, x1, half-open
    b = torch.from_numpy(rects).to(dev)
    ys = torch.arange(H, device=dev)[None, :, None]
    xs = torch.arange(W, device=dev)[None, None, :]
    masks = (ys >= b[:, 0, None, None]) & (ys < b[:, 1, None, None]) & (xs >= b[:, 2, None, None]) & (xs < b[:, 3, None, None])
    boxes = np.stack([rects[:, 2], rects[:, 0], rects[:, 3] - rects[:, 2], rects[:, 1] - rects[:, 0]], axis=1)
    image = np.random.RandomState(seed + 17).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    return masks.contiguous(), torch.from_numpy(boxes.astype(np.int32)).to(dev), torch.from_numpy(image).to(dev)


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def torch_tiles(image, masks, host_boxes, mean, std):
    """Baseline (a): (n, 3, S, S) float16 and the 0 .. 255 float tiles."""
    tiles = []
    zero = torch.zeros((), dtype=torch.uint8, device=image.device)
    for m, (x, y, w, h) in zip(masks, host_boxes):
        seg = torch.where(m[..., None], image, zero)[y:y + h, x:x + w]
        l = max(w, h)
        pad = torch.zeros((l, l, 3), dtype=torch.uint8, device=image.device)
        if h > w:
            pad[:, (h - w) // 2:(h - w) // 2 + w] = seg
        else:
            pad[(w - h) // 2:(w - h) // 2 + h] = seg
        tiles.append(F.interpolate(pad.permute(2, 0, 1)[None].float(), size=(S, S), mode="bilinear",
                                   align_corners=False)[0])
    t255 = torch.stack(tiles)
    return ((t255 / 255.0 - mean) / std).half(), t255


def host_steps(image, masks, host_boxes, dev):
    """Baseline (b): seconds for the reference's host steps without the resize."""
    t0 = time.perf_counter()
    for m, (x, y, w, h) in zip(masks, host_boxes):
        img = image.copy()
        img[m == 0] = np.array([0, 0, 0], dtype=np.uint8)
        seg = img[y:y + h, x:x + w]
        l = max(w, h)
        pad = np.zeros((l, l, 3), dtype=np.uint8)
        if h > w:
            pad[:, (h - w) // 2:(h - w) // 2 + w] = seg
        else:
            pad[(w - h) // 2:(w - h) // 2 + h] = seg
    stack = np.zeros((len(masks), S, S, 3), dtype=np.uint8)   # where the resized squares would go
    up = (torch.from_numpy(stack.astype("float32")).permute(0, 3, 1, 2) / 255.0).to(dev)
    torch.cuda.synchronize()
    del up
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clip_tiles: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    mean = torch.tensor(CT.CLIP_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(CT.CLIP_STD, device=dev).view(1, 3, 1, 1)
    lines = []
    for N, H, W in SHAPES:
        masks, boxes, image = scene(N, H, W, dev)
        packed = MN.pack_masks(masks)
        host_boxes = [tuple(int(v) for v in b) for b in boxes.cpu().numpy()]
        boxes_equal = bool(torch.equal(CT.mask_boxes(packed), boxes))   # the scene's boxes are tight
        diff255 = None
        if not a.hip_only:
            u8 = CT.clip_tiles(image, packed, boxes, out="u8")
            ref16, ref255 = torch_tiles(image, masks, host_boxes, mean, std)
            diff255 = float((u8.permute(0, 3, 1, 2).float() - ref255).abs().max())
            del u8, ref16, ref255
        runs = {k: [] for k in ("boxes", "u8", "unit", "clip", "end_to_end", "torch")}

        def end_to_end():
            CT.clip_tiles(image, packed, CT.mask_boxes(packed), out="clip")

        for _ in range(3):   # alternate the variants so a busy neighbour hits all alike
            runs["boxes"].append(timed(lambda: CT.mask_boxes(packed), a.iters))
            if not a.hip_only:
                runs["torch"].append(timed(lambda: torch_tiles(image, masks, host_boxes, mean, std), a.torch_iters,
                                           warmup=1))
            for form in ("u8", "unit", "clip"):
                runs[form].append(timed(lambda: CT.clip_tiles(image, packed, boxes, out=form), a.iters))
            runs["end_to_end"].append(timed(end_to_end, a.iters))
        best = {k: min(v) for k, v in runs.items() if v}
        W64 = (H * W + 63) // 64
        shape = {"N": N, "H": H, "W": W, "tile": S}
        box_bytes = N * W64 * 8
        hip = {"variant": "hip", **shape, "ms_mask_boxes": round(best["boxes"], 4),
               "mask_boxes_read_GBps": round(box_bytes / best["boxes"] / 1e6, 1),
               "mask_boxes_time_over_floor": round(best["boxes"] * 1e-3 / (box_bytes / PEAK_BPS), 2),
               "mask_boxes_equal_scene_boxes": boxes_equal}
        for form in ("u8", "unit", "clip"):
            out_bytes = N * S * S * 3 * ELEM[form]
            hip[f"ms_clip_tiles_{form}"] = round(best[form], 4)
            hip[f"clip_tiles_{form}_write_GBps"] = round(out_bytes / best[form] / 1e6, 1)
            hip[f"clip_tiles_{form}_time_over_floor"] = round(best[form] * 1e-3 / (out_bytes / PEAK_BPS), 2)
        hip["ms_end_to_end_boxes_then_clip"] = round(best["end_to_end"], 4)
        hip["floor_bytes_per_s"] = PEAK_BPS
        hip["ms_runs"] = {k: [round(t, 4) for t in v] for k, v in runs.items() if k != "torch"}
        lines.append(hip)
        print(json.dumps(hip), flush=True)
        if a.hip_only:
            continue
        lines.append({"variant": "torch", **shape, "bit_equal": False,
                      "note": "per mask: where, crop, pad, F.interpolate(bilinear, align_corners=False); float bilinear, not bit-equal",
                      "ms_tiles_clip_form": round(best["torch"], 3),
                      "ratio_torch_over_hip_clip": round(best["torch"] / best["clip"], 1),
                      "max_abs_diff_of_0_255_tiles": round(diff255, 3),
                      "ms_runs": [round(t, 3) for t in runs["torch"]]})
        secs = host_steps(image.cpu().numpy(), masks.cpu().numpy(), host_boxes, dev)
        lines.append({"variant": "host_steps", **shape, "host_work": True, "resize_left_out": True,
                      "note": "frame copy, masked write, crop, pad per mask; float stack / 255; upload: a lower bound on the reference's time",
                      "ms_measured_once": round(secs * 1e3, 1),
                      "ratio_host_over_hip_unit": round(secs * 1e3 / best["unit"], 0)})
        for ln in lines[-2:]:
            print(json.dumps(ln), flush=True)
        del masks, packed, image
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(ln) for ln in lines) + "\n")


if __name__ == "__main__":
    main()
