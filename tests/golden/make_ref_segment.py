"""Generate tests/golden/ref_segment.npz by running the REFERENCE's own
segmentation_process_cuda (eval_lerf.py:111-156) and localization_process_cuda
(eval_lerf.py:158-200) on seeded relevancy maps, on the CPU.

eval_lerf imports the whole evaluation stack at its top (the renderer, the
scene loader, cv2, torchvision, open_clip, mediapy, ...); none of it is used by
the two functions, so every module that cannot be imported here is replaced by
an empty stand-in whose attributes are inert placeholders (for generation
only).  The clip_model both functions receive is a SimpleNamespace whose
get_max_across_quick returns a prepared float64 (3, 3, 24, 40) tensor — values
that are exactly representable in fp32, so the fp32 kernels and this float64
evaluation start from the same numbers.  segmentation_process_cuda blends that
tensor in place (eval_lerf.py:126), so the blended maps are read back from it;
localization_process_cuda gets a fresh copy.

Stored: the input, the annotation masks and boxes, the blended maps, the
reference's chosen_iou_list / chosen_lvl_list and its acc_num.

Run:  python tests/golden/make_ref_segment.py   (needs the reference tree,
LSR_REFERENCE or /root/reference; only the .npz is committed).
"""
import importlib
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

REF = os.environ.get("LSR_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_segment.npz")
THRESH = 0.4


class _Placeholder:
    """What a stand-in module hands out for any name: callable, subclassable, inert."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return self

    def __class_getitem__(cls, item):
        return cls

    def __getattr__(self, name):
        return _Placeholder()


class _Stub(types.ModuleType):
    __path__ = []   # a package, so its submodules are looked up (and stubbed in turn)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Placeholder


def import_eval_lerf():
    sys.path.insert(0, REF)
    stubbed = []
    for _ in range(200):
        try:
            return importlib.import_module("eval_lerf"), stubbed
        except ModuleNotFoundError as e:
            sys.modules[e.name] = _Stub(e.name)
            stubbed.append(e.name)
            for k in [k for k in sys.modules if k == "eval_lerf" or k.split(".")[0] in ("eval", "scene", "utils",
                                                                                       "gaussian_renderer",
                                                                                       "arguments")]:
                if not isinstance(sys.modules[k], _Stub):
                    del sys.modules[k]   # half-imported reference modules are imported afresh
    raise RuntimeError("could not import eval_lerf")


def gauss_blur(a, sigma):
    r = max(1, int(3 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    a = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="reflect"), k, mode="valid"), -1, a)
    return np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="reflect"), k, mode="valid"), -2, a)


def field(g, shape, sigma):
    """Relevancy-like planes in (0, 1): a sigmoid of smooth noise plus a little white noise."""
    z = gauss_blur(g.standard_normal(shape), sigma)
    z = 3.0 * z / z.std(axis=(-2, -1), keepdims=True)
    v = 0.96 / (1.0 + np.exp(-z)) + 0.02 + 0.02 * (g.random(shape) - 0.5)
    return v.astype(np.float32)


def main():
    eval_lerf, stubbed = import_eval_lerf()
    g = np.random.default_rng(20240712)
    L, Q, H, W = 3, 3, 24, 40
    rel = field(g, (L, Q, H, W), 3.0)
    prompts = [f"prompt{q}" for q in range(Q)]
    # annotation masks: a rectangle around each prompt's hottest region at level 1, one left empty;
    # boxes: two per prompt, corners in either order
    gt = np.zeros((Q, H, W), np.uint8)
    boxes = np.zeros((Q, 2, 4), np.float64)
    for q in range(Q):
        y, x = np.unravel_index(np.argmax(rel[1, q]), (H, W))
        if q != 2:
            gt[q, max(0, y - 5):y + 6, max(0, x - 7):x + 8] = 1
        boxes[q, 0] = (x + 9, y + 7, x - 9, y - 7)            # x1 y1 x2 y2, swapped corners
        boxes[q, 1] = (0, 0, 3, 2)
    img_ann = {p: {"mask": gt[q], "bboxes": boxes[q]} for q, p in enumerate(prompts)}

    vm = torch.from_numpy(rel).double()
    model = SimpleNamespace(get_max_across_quick=lambda sem_map: vm)
    with torch.no_grad():
        ious, lvls = eval_lerf.segmentation_process_cuda(None, model, THRESH, img_ann, prompts)
        blended = vm.numpy().copy()
        vm2 = torch.from_numpy(rel).double()
        model2 = SimpleNamespace(get_max_across_quick=lambda sem_map: vm2)
        acc = eval_lerf.localization_process_cuda(None, model2, img_ann)
    assert np.array_equal(vm2.numpy(), rel.astype(np.float64))   # the localisation does not write its input
    assert not np.array_equal(blended, rel.astype(np.float64))
    np.savez_compressed(OUT, rel=rel, gt_masks=gt, boxes=boxes, thresh=np.float64(THRESH), blended=blended,
                        chosen_iou_list=np.asarray(ious, np.float64), chosen_lvl_list=np.asarray(lvls, np.int64),
                        acc_num=np.int64(acc))
    print("stand-ins for:", ", ".join(stubbed))
    print("wrote", OUT, os.path.getsize(OUT), "bytes; ious", ious, "levels", lvls, "acc_num", acc)


if __name__ == "__main__":
    main()
