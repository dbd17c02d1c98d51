"""Generate tests/golden/ref_mask_nms.npz by running the REFERENCE's own mask_nms
(preprocess.py:215-279) on the CPU over seeded rectangle scenes.  Pins
langsplatv2_amd/mask_nms.py and the float32 restatement in
tests/test_mask_nms.py to the reference, quirks included.

preprocess.py cannot be imported (it pulls in SAM and cv2), so the mask_nms
function node is taken out of its source with `ast` at run time and executed
with torch alone.  No reference text is stored, only data: per case the masks
as packed bits (numpy.packbits, little bit order, one row per mask), the
float64 scores and the reference's selected_idx; and the thresholds of the
reference's call site (preprocess.py:302).

A scene (rect_scene) is N axis-aligned boxes, each one of: a fresh box; a
near-duplicate of an earlier box (every edge moved by -1, 0 or +1 px); a
half-size box inside an earlier one; a 1-5 px speck.  Scores are a permutation
of N distinct values in [0.4, 1.0], so ties cannot arise (the reference's sort
is unstable).  tools/bench_mask_nms.py draws its larger scenes from the same
generator.

Run:  LSR_REFERENCE=<reference checkout> python tests/golden/make_ref_mask_nms.py
(only the resulting .npz is committed and travels)."""
import ast
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_mask_nms.npz")
THRESHOLDS = dict(iou_thr=0.8, score_thr=0.7, inner_thr=0.5)   # preprocess.py:302
SHAPES = [(5, 8, 9), (33, 40, 56), (64, 65, 130), (97, 48, 70)]
SEEDS = (0, 1, 2)


def rect_boxes(N, H, W, seed):
    """N boxes (y0, y1, x0, x1), half-open, and (N,) float64 scores."""
    rng = np.random.RandomState(1000003 * seed + 1009 * N + 31 * H + W)
    boxes = []   # y0, y1, x0, x1 (half-open)
    for n in range(N):
        kind = rng.choice(4, p=[0.4, 0.2, 0.25, 0.15]) if boxes else 0
        if kind == 0:      # a fresh box
            h = rng.randint(max(2, H // 8), max(3, H // 2) + 1)
            w = rng.randint(max(2, W // 8), max(3, W // 2) + 1)
            y0, x0 = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
            box = (y0, y0 + h, x0, x0 + w)
        elif kind == 1:    # an earlier box with every edge moved by at most one pixel
            y0, y1, x0, x1 = boxes[rng.randint(len(boxes))]
            d = rng.randint(-1, 2, size=4)
            y0, x0 = min(max(y0 + d[0], 0), H - 1), min(max(x0 + d[2], 0), W - 1)
            box = (y0, min(max(y1 + d[1], y0 + 1), H), x0, min(max(x1 + d[3], x0 + 1), W))
        elif kind == 2:    # half the height and width, inside an earlier box
            y0, y1, x0, x1 = boxes[rng.randint(len(boxes))]
            h, w = max(1, (y1 - y0) // 2), max(1, (x1 - x0) // 2)
            yy, xx = rng.randint(y0, y1 - h + 1), rng.randint(x0, x1 - w + 1)
            box = (yy, yy + h, xx, xx + w)
        else:              # a speck: a run of 1-5 px in one row
            k = min(rng.randint(1, 6), W)
            yy, xx = rng.randint(0, H), rng.randint(0, W - k + 1)
            box = (yy, yy + 1, xx, xx + k)
        boxes.append(box)
    scores = np.linspace(0.4, 1.0, N)[rng.permutation(N)] if N > 1 else np.array([0.9])
    return np.array(boxes, dtype=np.int64), scores.astype(np.float64)


def rect_scene(N, H, W, seed):
    """(N, H, W) bool masks and (N,) float64 scores."""
    boxes, scores = rect_boxes(N, H, W, seed)
    masks = np.zeros((N, H, W), dtype=bool)
    for n, (y0, y1, x0, x1) in enumerate(boxes):
        masks[n, y0:y1, x0:x1] = True
    return masks, scores


def hand_cases():
    one = np.zeros((1, 3, 5), dtype=bool)
    one[0, 0:2, 1:4] = True
    two = np.zeros((2, 3, 5), dtype=bool)
    two[0, 0:2, 0:3] = True
    two[1, 1:3, 2:5] = True
    return {"hand_1x3x5": (one, np.array([0.9])), "hand_2x3x5": (two, np.array([0.8, 0.9]))}


def pack_bits(masks):
    return np.packbits(masks.reshape(masks.shape[0], -1), axis=1, bitorder="little")


def reference_mask_nms(reference):
    """The reference's mask_nms, compiled from its function node alone."""
    import torch
    path = os.path.join(reference, "preprocess.py")
    tree = ast.parse(open(path).read(), filename=path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "mask_nms")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["mask_nms"]


def main():
    import torch
    if not os.environ.get("LSR_REFERENCE"):
        sys.exit("set LSR_REFERENCE to the reference checkout (the directory holding preprocess.py)")
    ref = reference_mask_nms(os.environ["LSR_REFERENCE"])
    cases = {f"rect_{N}x{H}x{W}_s{s}": rect_scene(N, H, W, s) for (N, H, W) in SHAPES for s in SEEDS}
    cases.update(hand_cases())
    out = {"thresholds": np.array([THRESHOLDS["iou_thr"], THRESHOLDS["score_thr"], THRESHOLDS["inner_thr"]]),
           "cases": np.array(sorted(cases))}
    for name in sorted(cases):
        masks, scores = cases[name]
        sel = ref(torch.from_numpy(masks), torch.from_numpy(scores), **THRESHOLDS).numpy().astype(np.int64)
        out[name + "_bits"] = pack_bits(masks)
        out[name + "_shape"] = np.array(masks.shape, dtype=np.int64)
        out[name + "_scores"] = scores
        out[name + "_selected"] = sel
        print(name, "keeps", len(sel), "of", len(scores))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
