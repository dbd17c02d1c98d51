"""Generate tests/golden/ref_clip_tiles.npz by running the REFERENCE's own
get_seg_img and pad_img (preprocess.py:191-206) on the CPU over seeded scenes.
Pins the crop-and-pad half of langsplatv2_amd/clip_tiles.py, and its numpy
restatement in tests/test_clip_tiles.py, to the reference.  The resize half is
cv2's and cv2 is not available here, so it is pinned by the restated integer
algorithm alone (DESIGN, "CLIP tiles").

preprocess.py cannot be imported (it pulls in SAM and cv2), so the two function
nodes are taken out of its source with `ast` at run time and executed with
numpy alone, as make_ref_mask_nms.py does.  No reference text is stored, only
data: per case the frame (H, W, 3) uint8, the masks as packed bits
(numpy.packbits, little bit order, one row per mask), the boxes after the
reference's np.int32 cast, and the padded squares (side l, l l 3 bytes each, one
after the other).

A scene is a seeded random frame and up to 6 hand-placed masks: rectangles,
some with random holes, an ellipse; boxes tight, larger than the mask, reaching
past the frame, with fractional coordinates (SAM's are floats), one of no width.

Run:  LSR_REFERENCE=<reference checkout> python tests/golden/make_ref_clip_tiles.py
(only the resulting .npz is committed and travels)."""
import ast
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_clip_tiles.npz")


def _rect(H, W, y0, y1, x0, x1, rng=None, p=1.0):
    m = np.zeros((H, W), dtype=bool)
    m[y0:y1, x0:x1] = True if rng is None else rng.random_sample((y1 - y0, x1 - x0)) < p
    return m


def scenes():
    """name -> (image (H, W, 3) uint8, masks (N, H, W) bool, bboxes: N lists x, y, w, h as SAM gives them)."""
    out = {}
    rng = np.random.RandomState(20240607)
    H, W = 40, 56
    image = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = [_rect(H, W, 5, 25, 8, 20),                       # taller than wide, solid
             _rect(H, W, 30, 37, 3, 50, rng, 0.7),            # wider than tall (odd difference), with holes
             ((yy - 18) / 9.0) ** 2 + ((xx - 38) / 11.0) ** 2 <= 1.0,   # an ellipse
             _rect(H, W, 0, 9, 0, 9),                         # in the corner, its box larger than the mask
             _rect(H, W, 31, 40, 44, 56, rng, 0.8),           # at the far corner, its box reaches past the frame
             _rect(H, W, 12, 13, 1, 4)]                       # a speck: l = 3
    boxes = [[8, 5, 12, 20], [3, 30, 47, 7], [27, 9, 23, 19], [0, 0, 15, 12], [40, 30, 30, 20], [1, 12, 3, 1]]
    out["a_40x56"] = (image, np.stack(masks), boxes)
    H, W = 65, 130
    image = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    masks = [_rect(H, W, 20, 53, 100, 118, rng, 0.9),         # 33 x 18: an odd difference
             _rect(H, W, 2, 14, 60, 97, rng, 0.5),            # 12 x 37, half of it holes
             _rect(H, W, 40, 49, 10, 20),                     # its box has no width: an all-zero square of side 9
             _rect(H, W, 20, 46, 70, 96, rng, 0.6),           # fractional box coordinates
             _rect(H, W, 64, 65, 129, 130)]                   # the last pixel of the frame: l = 1
    boxes = [[100.0, 20.0, 18.0, 33.0], [60.0, 2.0, 37.0, 12.0], [12, 40, 0, 9], [70.7, 20.2, 25.9, 25.1],
             [129.0, 64.0, 1.0, 1.0]]
    out["b_65x130"] = (image, np.stack(masks), boxes)
    return out


def pack_bits(masks):
    return np.packbits(masks.reshape(masks.shape[0], -1), axis=1, bitorder="little")


def reference_functions(reference):
    """The reference's get_seg_img and pad_img, compiled from their function nodes alone."""
    path = os.path.join(reference, "preprocess.py")
    tree = ast.parse(open(path).read(), filename=path)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("get_seg_img", "pad_img")]
    assert len(nodes) == 2
    ns = {"np": np}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns["get_seg_img"], ns["pad_img"]


def main():
    if not os.environ.get("LSR_REFERENCE"):
        sys.exit("set LSR_REFERENCE to the reference checkout (the directory holding preprocess.py)")
    get_seg_img, pad_img = reference_functions(os.environ["LSR_REFERENCE"])
    cases = scenes()
    out = {"cases": np.array(sorted(cases))}
    for name in sorted(cases):
        image, masks, bboxes = cases[name]
        squares = [pad_img(get_seg_img({"segmentation": m, "bbox": b}, image)) for m, b in zip(masks, bboxes)]
        assert all(s.dtype == np.uint8 and s.shape == (s.shape[0], s.shape[0], 3) for s in squares)
        out[name + "_image"] = image
        out[name + "_bits"] = pack_bits(masks)
        out[name + "_shape"] = np.array(masks.shape, dtype=np.int64)
        out[name + "_boxes"] = np.stack([np.int32(b) for b in bboxes])
        out[name + "_sides"] = np.array([s.shape[0] for s in squares], dtype=np.int32)
        out[name + "_squares"] = np.concatenate([s.reshape(-1) for s in squares])
        print(name, "sides", [s.shape[0] for s in squares])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
