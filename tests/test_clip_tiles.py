"""langsplatv2_amd/clip_tiles.py: the CLIP input tiles of the kept SAM masks
(csrc/clip_tiles.hip, C ABI lsr_mask_boxes / lsr_clip_tiles), replacing the tile
half of mask2segmap (preprocess.py:304-317 with get_seg_img :191-196 and pad_img
:198-206), the / 255 of :315 and encode_image's normalisation and cast (:105-107).

The chain of evidence:

  reference's own get_seg_img and pad_img (run by tests/golden/make_ref_clip_tiles.py)
      == tests/golden/ref_clip_tiles.npz
      == `restate_square` below                                                      [CPU test]
  `restate_resize` below, OpenCV's 8-bit INTER_LINEAR arithmetic in integers as read
      from its source (never compared with a cv2 build: there is none here):
      the identity at l == S, the 2 x 2 box average at l == 2 S, and within 1.26 of
      exact float64 bilinear interpolation with edge clamp                           [CPU tests]
  the HIP path == restate_resize(restate_square), bytewise for "u8" and bitwise for
      "unit" and "clip" against torch's own ops on the restated bytes                [GPU tests]

The bound 1.26 is derived, not fitted.  Against exact bilinear with the same
taps: each of the two coefficient pairs is rounded to 1 / 2048, at most
0.5 / 2048 per coefficient, and a pair's two errors weigh pixel values up to 255
(2 x 0.5 / 2048 x 255 = 0.1245 per pair, horizontal and vertical); `>> 4` drops
under 16 / 2048 = 0.008 of a pixel value; each of the two `>> 16` drops under one
unit of a quantity that the final `>> 2` divides by 4, so under 1/4 each; and
the final (x + 2) >> 2 rounds half up, at most 1/2.  Sum: 0.249 + 0.008 + 0.5 +
0.5 = 1.257 < 1.26.  The worst seen on the CPU is 0.82.
"""
import ctypes
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from langsplatv2_amd import _lib

# the package also exports the functions clip_tiles and mask_nms under their modules' names
CT = importlib.import_module("langsplatv2_amd.clip_tiles")
MN = importlib.import_module("langsplatv2_amd.mask_nms")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ref_clip_tiles.npz")
MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073])   # preprocess.py:42
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711])   # preprocess.py:43
BOUND = 1.26


@functools.lru_cache(maxsize=None)
def fixture():
    """name -> (image (H, W, 3) uint8, masks (N, H, W) bool, boxes (N, 4) int32, squares: list of (l, l, 3) uint8);
    shared, never modified."""
    z = np.load(GOLD)
    out = {}
    for name in z["cases"]:
        name = str(name)
        N, H, W = (int(v) for v in z[name + "_shape"])
        masks = np.unpackbits(z[name + "_bits"], axis=1, bitorder="little")[:, :H * W].reshape(N, H, W).astype(bool)
        sides, flat, squares, at = z[name + "_sides"], z[name + "_squares"], [], 0
        for l in sides:
            squares.append(flat[at:at + 3 * l * l].reshape(l, l, 3))
            at += 3 * l * l
        assert at == flat.shape[0]
        out[name] = (z[name + "_image"], masks, z[name + "_boxes"], squares)
    return out


FIXTURE_NAMES = sorted(str(n) for n in np.load(GOLD)["cases"])


# ----------------------------------------------------------- restatement ---
def crop_of(box, H, W):
    """The box clipped to the frame as numpy slicing clips it (a negative origin clamped): x0, y0, cw, ch."""
    x, y, w, h = (int(v) for v in box)
    x0, x1 = min(max(x, 0), W), min(max(x + w, 0), W)
    y0, y1 = min(max(y, 0), H), min(max(y + h, 0), H)
    return x0, y0, max(x1 - x0, 0), max(y1 - y0, 0)


def restate_square(image, mask, box):
    """get_seg_img then pad_img: the (l, l, 3) uint8 square of one mask."""
    H, W = mask.shape
    x0, y0, cw, ch = crop_of(box, H, W)
    l = max(cw, ch)
    sq = np.zeros((l, l, 3), dtype=np.uint8)
    crop = image[y0:y0 + ch, x0:x0 + cw] * mask[y0:y0 + ch, x0:x0 + cw, None].astype(np.uint8)
    if ch > cw:
        sq[:, (ch - cw) // 2:(ch - cw) // 2 + cw] = crop
    else:
        sq[(cw - ch) // 2:(cw - ch) // 2 + ch, :] = crop
    return sq


def resize_tables(l, S):
    """Taps and 11-bit coefficients of the l -> S resize: horizontal (c0, c1, a0, a1), vertical (r0, r1, b0, b1)."""
    scale = 1.0 / (float(S) / float(l))
    f = ((np.arange(S, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = f - s                                  # float32
    assert f.dtype == np.float32
    s = s.astype(np.int64)
    one, k = np.float32(1.0), np.float32(2048.0)
    fh, sh = f.copy(), s.copy()
    fh[sh < 0], sh[sh < 0] = 0, 0
    fh[sh >= l - 1], sh[sh >= l - 1] = 0, l - 1
    a1, a0 = np.rint(fh * k).astype(np.int64), np.rint((one - fh) * k).astype(np.int64)
    b1, b0 = np.rint(f * k).astype(np.int64), np.rint((one - f) * k).astype(np.int64)
    return (sh, np.minimum(sh + 1, l - 1), a0, a1), (np.clip(s, 0, l - 1), np.clip(s + 1, 0, l - 1), b0, b1)


def restate_resize(sq, S):
    """OpenCV's generic 8-bit INTER_LINEAR path, l x l x 3 -> S x S x 3, in integers."""
    l = sq.shape[0]
    if l == 0:
        return np.zeros((S, S, 3), dtype=np.uint8)
    (c0, c1, a0, a1), (r0, r1, b0, b1) = resize_tables(l, S)
    q = sq.astype(np.int64)
    h0 = q[r0][:, c0] * a0[None, :, None] + q[r0][:, c1] * a1[None, :, None]
    h1 = q[r1][:, c0] * a0[None, :, None] + q[r1][:, c1] * a1[None, :, None]
    p0, p1 = b0[:, None, None] * (h0 >> 4), b1[:, None, None] * (h1 >> 4)
    assert max(h0.max(), h1.max(), p0.max(), p1.max()) < 2 ** 31     # every product fits int32
    out = ((p0 >> 16) + (p1 >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255                       # no saturation needed
    return out.astype(np.uint8)


def exact_bilinear(sq, S):
    """float64 bilinear interpolation at the same sample points, indices clamped to the edge."""
    l = sq.shape[0]
    x = (np.arange(S, dtype=np.float64) + 0.5) * (l / S) - 0.5
    i0 = np.floor(x)
    f = x - i0
    j0, j1 = np.clip(i0, 0, l - 1).astype(np.int64), np.clip(i0 + 1, 0, l - 1).astype(np.int64)
    q = sq.astype(np.float64)
    rows = q[j0] * (1 - f)[:, None, None] + q[j1] * f[:, None, None]
    return rows[:, j0] * (1 - f)[None, :, None] + rows[:, j1] * f[None, :, None]


def restate_tiles(image, masks, boxes, keep, S):
    """(n, S, S, 3) uint8: tile t is mask keep[t] (None: all, in order)."""
    idx = range(len(masks)) if keep is None else keep
    tiles = [restate_resize(restate_square(image, masks[i], boxes[i]), S) for i in idx]
    return np.stack(tiles) if tiles else np.zeros((0, S, S, 3), dtype=np.uint8)


def float_forms(u8):
    """torch's own ops on the restated bytes: mask2segmap's seg_imgs and encode_image's input."""
    unit = (torch.from_numpy(u8).permute(0, 3, 1, 2) / 255.0).contiguous()
    clip = ((unit - MEAN.view(1, 3, 1, 1)) / STD.view(1, 3, 1, 1)).half()
    return unit, clip


def np_extents(masks):
    out = np.zeros((len(masks), 4), dtype=np.int32)
    for i, m in enumerate(masks):
        ys, xs = np.where(m)
        if len(ys):
            out[i] = (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
    return out


def random_image(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


def random_masks(N, H, W, seed, p=0.7):
    return np.random.RandomState(seed).random_sample((N, H, W)) < p


# ------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_restated_square_equals_reference(name):
    image, masks, boxes, squares = fixture()[name]
    assert len(squares) == len(masks)
    for i, want in enumerate(squares):
        got = restate_square(image, masks[i], boxes[i])
        assert got.shape == want.shape and np.array_equal(got, want), (name, i)


def test_fixture_holds_the_shapes_it_is_built_for():
    kinds = set()
    for name in FIXTURE_NAMES:
        image, masks, boxes, squares = fixture()[name]
        H, W = masks.shape[1:]
        assert H <= 65 and W <= 130 and len(masks) <= 6
        for m, b, sq in zip(masks, boxes, squares):
            x0, y0, cw, ch = crop_of(b, H, W)
            kinds.add("tall" if ch > cw else "wide" if cw > ch else "square")
            if abs(ch - cw) % 2:
                kinds.add("odd")
            if b[0] + b[2] > W or b[1] + b[3] > H:
                kinds.add("clipped")
            if cw == 0 and ch > 0:
                kinds.add("no_width")
                assert not sq.any()
            if (m[y0:y0 + ch, x0:x0 + cw] == 0).any():
                kinds.add("holes")
            if not np.array_equal(np_extents(m[None])[0], b):
                kinds.add("loose_box")
    assert kinds >= {"tall", "wide", "square", "odd", "clipped", "no_width", "holes", "loose_box"}, kinds


def test_resize_is_the_identity_at_equal_size():
    rng = np.random.RandomState(0)
    for l in (1, 2, 16, 224):
        sq = rng.randint(0, 256, size=(l, l, 3)).astype(np.uint8)
        assert np.array_equal(restate_resize(sq, l), sq), l


def test_resize_is_the_box_average_at_half_size():
    rng = np.random.RandomState(1)
    for S in (1, 3, 16, 112):
        sq = rng.randint(0, 256, size=(2 * S, 2 * S, 3)).astype(np.uint8)
        q = sq.astype(np.int64)
        want = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2
        assert np.array_equal(restate_resize(sq, S), want.astype(np.uint8)), S


def test_resize_is_close_to_exact_bilinear():
    rng = np.random.RandomState(2)
    worst = 0.0
    for S in (8, 16, 224):
        for l in (1, 2, 3, 5, 7, 15, 16, 17, 31, 33, 100, 223, 225, 449, 600):
            for kind in range(2):   # uniform noise; black and white only (the largest steps)
                sq = rng.randint(0, 256, size=(l, l, 3)) if kind == 0 else 255 * rng.randint(0, 2, size=(l, l, 3))
                sq = sq.astype(np.uint8)
                got = restate_resize(sq, S)
                err = np.abs(got.astype(np.float64) - exact_bilinear(sq, S)).max()
                worst = max(worst, err)
                assert err < BOUND, (l, S, kind, err)
    print("worst |restate - exact bilinear| =", worst)


def test_the_two_tables_share_the_floor_and_differ_at_the_edges():
    (c0, c1, a0, a1), (r0, r1, b0, b1) = resize_tables(3, 16)   # upscaling: the first source coordinate is below 0
    assert (c0[0], c1[0], a0[0], a1[0]) == (0, 1, 2048, 0)      # horizontal: f forced to 0
    assert (r0[0], r1[0]) == (0, 0) and b1[0] != 0              # vertical: both rows clamped, f kept
    assert (c0[-1], c1[-1], a1[-1]) == (2, 2, 0) and (r0[-1], r1[-1]) == (2, 2) and b1[-1] != 0
    inner = (r0 == c0) & (r1 == r0 + 1) & (c1 == c0 + 1)        # 0 <= floor(f) <= l - 2: no edge rule applies
    assert np.array_equal(a0[inner], b0[inner]) and np.array_equal(a1[inner], b1[inner]) and inner.sum() >= 8


def test_c_abi_argument_checks():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 1024)()
    P = (ctypes.addressof(buf) + 255) & ~255   # a 256-B aligned stand-in address, never dereferenced
    OK, EINVAL = 0, 1
    big_h, big_w = 4096, 4097   # H W = 2^24 + 4096
    for args, want in [                      # lsr_mask_boxes(words, N, H, W, boxes, stream)
            ((None, 5, 3, 5, P, None), EINVAL), ((P, 5, 3, 5, None, None), EINVAL), ((P + 4, 5, 3, 5, P, None), EINVAL),
            ((P, 5, 3, 5, P + 2, None), EINVAL), ((P, -1, 3, 5, P, None), EINVAL), ((P, 4097, 3, 5, P, None), EINVAL),
            ((P, 5, 0, 5, P, None), EINVAL), ((P, 5, 3, 0, P, None), EINVAL), ((P, 5, big_h, big_w, P, None), EINVAL),
            ((None, 0, 0, 5, None, None), EINVAL), ((None, 0, 3, 5, None, None), OK)]:
        assert lib.lsr_mask_boxes(*args) == want, args
    # lsr_clip_tiles(image, H, W, words, N, keep, boxes, n, S, lut, out_type, out, stream)
    good = [P, 3, 5, P, 5, P, P, 4, 8, P, 2, P, None]
    for pos in (0, 3, 6, 9, 11):                 # each required pointer (lut: a float form)
        args = list(good)
        args[pos] = None
        assert lib.lsr_clip_tiles(*args) == EINVAL, pos
    for pos, val in [(1, 0), (2, 0), (1, -3), (4, -1), (4, 4097), (7, -1), (7, 4097), (8, 0), (8, 1025), (8, -224),
                     (10, 3), (10, -1), (3, P + 4), (5, P + 2), (6, P + 2), (9, P + 1), (11, P + 1)]:
        args = list(good)
        args[pos] = val
        assert lib.lsr_clip_tiles(*args) == EINVAL, (pos, val)
    args = list(good)
    args[1], args[2] = big_h, big_w
    assert lib.lsr_clip_tiles(*args) == EINVAL
    args = list(good)
    args[5], args[7] = None, 6                   # without keep the tiles are the first n masks: n <= N
    assert lib.lsr_clip_tiles(*args) == EINVAL
    args = list(good)
    args[9], args[10], args[11] = None, 0, None  # "u8" needs no table, but an output
    assert lib.lsr_clip_tiles(*args) == EINVAL
    args = list(good)
    args[10], args[11] = 1, P + 2                # fp32 output on a 2-B boundary
    assert lib.lsr_clip_tiles(*args) == EINVAL
    assert lib.lsr_clip_tiles(None, 3, 5, None, 5, None, None, 0, 224, None, 2, None, None) == OK   # n = 0: a no-op
    assert lib.lsr_clip_tiles(None, 3, 5, None, 0, None, None, 0, 224, None, 0, None, None) == OK
    assert lib.lsr_clip_tiles(None, 0, 5, None, 5, None, None, 0, 224, None, 2, None, None) == EINVAL  # the shape first


def test_python_argument_errors():
    masks = torch.zeros((3, 4, 5), dtype=torch.bool)
    image = torch.zeros((4, 5, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        CT.mask_boxes(masks)
    with pytest.raises(RuntimeError, match="image must be a ROCm device tensor .there is no CPU path"):
        CT.clip_tiles(image, masks)
    cpu_packed = MN.PackedMasks(torch.zeros((3, 1), dtype=torch.int64), torch.zeros(3, dtype=torch.int32), 4, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        CT.mask_boxes(cpu_packed)
    with pytest.raises(ValueError, match="3-D"):
        CT.mask_boxes(masks[0])
    with pytest.raises(ValueError, match=r"image must be a 3-D tensor \(H, W, 3\)"):
        CT.clip_tiles(image[..., 0], masks)
    with pytest.raises(ValueError, match=r"image must be a 3-D tensor \(H, W, 3\)"):
        CT.clip_tiles(image.permute(2, 0, 1), masks)
    with pytest.raises(ValueError, match="image must be uint8"):
        CT.clip_tiles(image.float(), masks)
    with pytest.raises(ValueError, match="masks must be a PackedMasks or a 3-D tensor"):
        CT.clip_tiles(image, masks[0])
    with pytest.raises(ValueError, match="out must be one of"):
        CT.clip_tiles(image, masks, out="float")
    for size in (0, 1025, 224.0):
        with pytest.raises(ValueError, match="size must be an integer in 1 .. 1024"):
            CT.clip_tiles(image, masks, size=size)
    with pytest.raises(ValueError, match="out must be"):
        CT.tile_lut("u8")
    with pytest.raises(ValueError, match="3 values"):
        CT.tile_lut("clip", mean=(0.5, 0.5))
    with pytest.raises(ValueError, match="no masks"):
        CT.mask2segmap([], np.zeros((4, 5, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="levels"):
        CT.segment_tiles_and_maps(np.zeros((4, 5, 3), dtype=np.uint8), [[]] * 5)
    with pytest.raises(ValueError, match="every level is empty"):
        CT.segment_tiles_and_maps(np.zeros((4, 5, 3), dtype=np.uint8), [[], []])


def test_lookup_tables_are_torchs_own_arithmetic():
    v = torch.arange(256, dtype=torch.uint8)
    unit = CT.tile_lut("unit")
    assert unit.dtype == torch.float32 and tuple(unit.shape) == (3, 256)
    assert all(torch.equal(unit[c].view(torch.int32), (v / 255.0).view(torch.int32)) for c in range(3))
    clip = CT.tile_lut("clip")
    assert clip.dtype == torch.float16 and tuple(clip.shape) == (3, 256)
    want = (((v / 255.0)[None, :] - MEAN[:, None]) / STD[:, None]).half()
    assert torch.equal(clip.view(torch.int16), want.view(torch.int16))
    assert tuple(CT.CLIP_MEAN) == tuple(float(x) for x in (0.48145466, 0.4578275, 0.40821073))
    assert tuple(CT.CLIP_STD) == tuple(float(x) for x in (0.26862954, 0.26130258, 0.27577711))


# ------------------------------------------------------------------- GPU ---
def check_tiles(gpu, image, masks, boxes, S, keep=None, what=""):
    """Every output form of the HIP path against the restatement; returns the restated bytes."""
    want = restate_tiles(image, masks, boxes, keep, S)
    unit, clip = float_forms(want)
    d_image = torch.from_numpy(image).to(gpu)
    d_masks = torch.from_numpy(np.ascontiguousarray(masks)).to(gpu)
    d_boxes = torch.from_numpy(np.asarray(boxes, dtype=np.int32).reshape(-1, 4)).to(gpu)
    d_keep = None if keep is None else torch.tensor(keep, dtype=torch.int64, device=gpu)
    n = len(want)
    got = CT.clip_tiles(d_image, d_masks, d_boxes, keep=d_keep, out="u8", size=S)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, S, S, 3), what
    bad = np.argwhere(got.cpu().numpy() != want)
    assert len(bad) == 0, (what, "u8", len(bad), bad[:4].tolist())
    got = CT.clip_tiles(d_image, d_masks, d_boxes, keep=d_keep, out="unit", size=S)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3, S, S), what
    assert torch.equal(got.cpu().view(torch.int32), unit.view(torch.int32)), (what, "unit")
    got = CT.clip_tiles(d_image, d_masks, d_boxes, keep=d_keep, out="clip", size=S, mean=MEAN, std=STD)
    assert got.dtype == torch.float16 and tuple(got.shape) == (n, 3, S, S), what
    assert torch.equal(got.cpu().view(torch.int16), clip.view(torch.int16)), (what, "clip")
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_fixture_scenes_at_the_default_size(gpu, name):
    image, masks, boxes, squares = fixture()[name]
    want = check_tiles(gpu, image, masks, boxes, 224, what=name)
    for i, sq in enumerate(squares):        # the reference's own squares, resized
        assert np.array_equal(want[i], restate_resize(sq, 224)), (name, i)


def edge_boxes(H, W):
    """x, y, w, h: every shape of crop the kernel treats differently."""
    return [(5, 2, 7, 20), (3, 10, 30, 9), (4, 4, 12, 12),      # taller than wide, wider than tall, square
            (9, 3, 6, 11), (9, 3, 11, 6), (2, 1, 8, 23),        # an odd difference either way: the // 2 offset
            (7, 7, 1, 1), (7, 7, 2, 1), (7, 7, 2, 2), (7, 7, 3, 2), (7, 7, 1, 3),   # l = 1, 2, 3
            (0, 6, 5, 9), (6, 0, 9, 5), (W - 5, 6, 5, 9), (6, H - 4, 9, 4),         # touching each frame edge
            (0, 0, W, H),                                       # the whole frame
            (W - 6, H - 5, 20, 30), (W - 3, 2, 40, 6),          # reaching past the frame: clipped
            (5, 5, 0, 7), (5, 5, 7, 0), (5, 5, 0, 0), (W, H, 4, 4),                 # no pixels: an all-zero tile
            (-3, -2, 10, 9)]                                    # a negative origin is clamped (numpy would wrap)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(40, 56), (65, 130), (48, 352)])
def test_box_shapes_on_small_tiles(gpu, hw):
    """W = 56 and 130: words straddle image rows; W = 352 with H W a multiple of 64: no word of a row group
    does at a row start that is a multiple of 64.  One mask per box, random with holes, so the bit decides."""
    H, W = hw
    boxes = edge_boxes(H, W)
    image = random_image(H, W, seed=H + W)
    masks = random_masks(len(boxes), H, W, seed=H * W)
    for S in (8, 16):
        want = check_tiles(gpu, image, masks, boxes, S, what=(hw, S))
        for i, b in enumerate(boxes):
            if b[2] <= 0 or b[3] <= 0 or b[0] >= W:
                assert not want[i].any(), (hw, S, b)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 7, 10, 300])
def test_tile_sides_off_the_fast_path(gpu, S):
    """S % 4 != 0 takes the element-wise stores and a partial last pixel group; S = 300 has more taps
    than a workgroup has threads and a partial last band of rows."""
    H, W = 40, 56
    boxes = [(5, 2, 7, 20), (3, 10, 30, 9), (0, 0, W, H), (7, 7, 1, 1)]
    check_tiles(gpu, random_image(H, W, seed=S), random_masks(len(boxes), H, W, seed=S + 1), boxes, S, what=S)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(1, 1), (1, 2), (2, 1), (1, 3)])
def test_frames_of_a_few_pixels(gpu, hw):
    """The kernel reads a pixel pair with one 8-byte load clamped into the frame's 3 H W bytes; frames
    under 8 bytes (one or two pixels) take byte loads, 9 bytes is the first that does not."""
    H, W = hw
    masks = np.ones((2, H, W), dtype=bool)
    masks[1, H - 1, W - 1] = False
    check_tiles(gpu, random_image(H, W, seed=10 + H + W), masks, [(0, 0, W, H), (0, 0, W, H)], 4, what=hw)


@pytest.mark.gpu
def test_equal_and_double_size_at_16(gpu):
    H, W, S = 40, 56, 16
    image, masks = random_image(H, W, seed=3), np.ones((2, H, W), dtype=bool)
    boxes = [(3, 3, 16, 16), (20, 5, 32, 32)]
    want = check_tiles(gpu, image, masks, boxes, S, what="l = S, 2 S")
    assert np.array_equal(want[0], image[3:19, 3:19])
    q = image[5:37, 20:52].astype(np.int64)
    assert np.array_equal(want[1], ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2))


@pytest.mark.gpu
def test_default_size_at_equal_side_and_past_double(gpu):
    H, W = 230, 240
    image, masks = random_image(H, W, seed=4), random_masks(1, H, W, seed=5, p=0.9)
    want = check_tiles(gpu, image, masks, [(5, 3, 224, 224)], 224, what="l = 224")
    assert np.array_equal(want[0], image[3:227, 5:229] * masks[0, 3:227, 5:229, None])
    H, W = 449, 37     # l = 449: the first non-integer downscale past 2 x
    image, masks = random_image(H, W, seed=6), random_masks(1, H, W, seed=7, p=0.9)
    check_tiles(gpu, image, masks, [(0, 0, W, H)], 224, what="l = 449")


@pytest.mark.gpu
def test_the_bit_decides_not_the_box(gpu):
    H, W, S = 40, 56, 16
    image = random_image(H, W, seed=8)
    masks = np.zeros((2, H, W), dtype=bool)
    masks[0, 10:30, 10:40] = True
    masks[0, 15:25, 20:30] = False          # a hole inside the box
    masks[1, 12:20, 30:41] = True           # its box is far larger than its extent
    want = check_tiles(gpu, image, masks, [(10, 10, 30, 20), (20, 5, 35, 33)], S, what="holes, loose box")
    tight = restate_tiles(image, masks, np_extents(masks), None, S)
    assert np.array_equal(want[0], tight[0]) and not np.array_equal(want[1], tight[1])
    solid = restate_tiles(image, np.ones_like(masks), [(10, 10, 30, 20), (20, 5, 35, 33)], None, S)
    assert not np.array_equal(want[0], solid[0]) and not np.array_equal(want[1], solid[1])


@pytest.mark.gpu
def test_keep_order_repeats_and_empty(gpu):
    image, masks, boxes, _ = fixture()["a_40x56"]
    want = check_tiles(gpu, image, masks, boxes, 16, keep=[3, 0, 3, 5, 1], what="keep")
    every = restate_tiles(image, masks, boxes, None, 16)
    assert np.array_equal(want, every[[3, 0, 3, 5, 1]])
    d_image, d_masks = torch.from_numpy(image).to(gpu), torch.from_numpy(masks).to(gpu)
    d_boxes = torch.from_numpy(boxes).to(gpu)
    for out, shape, dtype in (("u8", (0, 16, 16, 3), torch.uint8), ("unit", (0, 3, 16, 16), torch.float32),
                              ("clip", (0, 3, 16, 16), torch.float16)):
        got = CT.clip_tiles(d_image, d_masks, d_boxes, keep=torch.empty(0, dtype=torch.int64, device=gpu), out=out,
                            size=16)
        assert tuple(got.shape) == shape and got.dtype == dtype
        got = CT.clip_tiles(d_image, d_masks[:0], out=out, size=16)
        assert tuple(got.shape) == shape and got.dtype == dtype
    # a keep entry outside [0, N) reads as an empty mask
    got = CT.clip_tiles(d_image, d_masks, d_boxes, keep=torch.tensor([6, -1, 2], device=gpu), out="u8", size=16)
    assert not got[:2].any() and np.array_equal(got[2].cpu().numpy(), every[2])


@pytest.mark.gpu
def test_packed_and_dense_input_and_default_boxes(gpu):
    image, masks, boxes, _ = fixture()["b_65x130"]
    d_image, d_masks = torch.from_numpy(image).to(gpu), torch.from_numpy(masks).to(gpu)
    d_boxes = torch.from_numpy(boxes).to(gpu)
    packed = MN.pack_masks(d_masks)
    for out in ("u8", "unit", "clip"):
        a = CT.clip_tiles(d_image, d_masks, d_boxes, out=out)
        b = CT.clip_tiles(d_image, packed, d_boxes.to(torch.int64), out=out)
        assert tuple(a.shape[-2:] if out != "u8" else a.shape[1:3]) == (224, 224)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), out
    # boxes=None: the tight extents
    got = CT.clip_tiles(d_image, packed, out="u8", size=16)
    assert np.array_equal(got.cpu().numpy(), restate_tiles(image, masks, np_extents(masks), None, 16))


@pytest.mark.gpu
def test_run_to_run_identical(gpu):
    image, masks, boxes, _ = fixture()["a_40x56"]
    d_image, d_masks = torch.from_numpy(image).to(gpu), torch.from_numpy(masks).to(gpu)
    d_boxes = torch.from_numpy(boxes).to(gpu)
    for out in ("u8", "unit", "clip"):
        a = CT.clip_tiles(d_image, d_masks, d_boxes, out=out)
        b = CT.clip_tiles(d_image, d_masks, d_boxes, out=out)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), out
    assert torch.equal(CT.mask_boxes(d_masks), CT.mask_boxes(d_masks))


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(3, 5), (40, 56), (65, 130), (48, 352)])
def test_mask_boxes_equal_numpy_extents(gpu, hw):
    H, W = hw
    masks = np.concatenate([random_masks(4, H, W, seed=H, p=0.3), random_masks(6, H, W, seed=W, p=0.002),
                            np.zeros((4, H, W), dtype=bool)])
    masks[10, H // 2, W // 3] = True                 # a single pixel
    masks[11, H - 1, W - 1] = True                   # the last pixel of the frame
    masks[12] = True                                 # the full frame
    want = np_extents(masks)                         # mask 13 stays empty: 0, 0, 0, 0
    assert tuple(want[12]) == (0, 0, W, H) and tuple(want[13]) == (0, 0, 0, 0) and tuple(want[10][2:]) == (1, 1)
    d_masks = torch.from_numpy(masks).to(gpu)
    for src in (d_masks, MN.pack_masks(d_masks)):
        got = CT.mask_boxes(src)
        assert got.dtype == torch.int32 and tuple(got.shape) == (14, 4)
        assert np.array_equal(got.cpu().numpy(), want)
    assert tuple(CT.mask_boxes(d_masks[:0]).shape) == (0, 4)


def sam_dicts(masks, boxes, scores):
    return [{"segmentation": masks[i], "bbox": [float(v) for v in boxes[i]], "predicted_iou": scores[i],
             "stability_score": np.float64(1.0)} for i in range(len(masks))]


@pytest.mark.gpu
def test_mask2segmap_drop_in(gpu):
    image, masks, boxes, _ = fixture()["a_40x56"]
    dicts = sam_dicts(masks, boxes, np.linspace(0.9, 0.8, len(masks)))
    d_image, d_masks = torch.from_numpy(image).to(gpu), torch.from_numpy(masks).to(gpu)
    seg_imgs, seg_map = CT.mask2segmap(dicts, image, device=gpu)
    unit, _ = float_forms(restate_tiles(image, masks, boxes, None, 224))
    assert seg_imgs.is_cuda and torch.equal(seg_imgs.cpu().view(torch.int32), unit.view(torch.int32))
    assert torch.equal(seg_imgs, CT.clip_tiles(d_image, d_masks, torch.from_numpy(boxes).to(gpu), out="unit"))
    want = -np.ones(image.shape[:2], dtype=np.int32)
    for i, m in enumerate(masks):
        want[m] = i
    assert isinstance(seg_map, np.ndarray) and seg_map.dtype == np.int32 and np.array_equal(seg_map, want)
    clip, _ = CT.mask2segmap(dicts, image, device=gpu, out="clip", size=16)
    assert torch.equal(clip, CT.clip_tiles(d_image, d_masks, torch.from_numpy(boxes).to(gpu), out="clip", size=16))


@pytest.mark.gpu
def test_segment_tiles_and_maps(gpu):
    site = dict(iou_thr=0.8, score_thr=0.7, inner_thr=0.5)   # preprocess.py:302
    image, masks, boxes, _ = fixture()["a_40x56"]
    rng = np.random.RandomState(9)
    masks_m = np.concatenate([masks, masks[:1]])             # a duplicate of mask 0 with a lower score: NMS drops it
    boxes_m = np.concatenate([boxes, boxes[:1]])
    scores = [np.linspace(0.95, 0.75, len(masks))[rng.permutation(len(masks))], None,
              np.linspace(0.95, 0.75, len(masks_m)), None]
    levels = [sam_dicts(masks, boxes, scores[0]), [], sam_dicts(masks_m, boxes_m, scores[2])]
    tiles, seg_maps, lengths = CT.segment_tiles_and_maps(image, levels, device=gpu, size=16, **site)
    assert sorted(tiles) == ["default", "m"]                 # the empty level is skipped
    d_image = torch.from_numpy(image).to(gpu)
    packs, keeps = [], []
    for name, m, b, s in (("default", masks, boxes, scores[0]), ("s", None, None, None),
                          ("m", masks_m, boxes_m, scores[2])):
        if m is None:
            packs.append(None)
            keeps.append(None)
            continue
        packed = MN.pack_masks(torch.from_numpy(m).to(gpu))
        kept = torch.sort(MN.mask_nms(packed, torch.from_numpy(s).to(gpu), **site)).values
        want = CT.clip_tiles(d_image, packed, torch.from_numpy(b).to(gpu), keep=kept, out="clip", size=16)
        assert tiles[name].dtype == torch.float16 and torch.equal(tiles[name], want), name
        _, clip = float_forms(restate_tiles(image, m, b, kept.tolist(), 16))
        assert torch.equal(tiles[name].cpu().view(torch.int16), clip.view(torch.int16)), name
        packs.append(packed)
        keeps.append(kept)
    assert 0 < len(keeps[2]) < len(masks_m)                  # the NMS did drop something
    want_maps, want_lengths = MN.build_seg_maps(packs, keeps)
    assert lengths == want_lengths == [len(keeps[0]), 0, len(keeps[2]), 0]
    assert seg_maps.dtype == torch.float32 and tuple(seg_maps.shape) == (4, 40, 56)
    assert torch.equal(seg_maps, want_maps)
    assert int(seg_maps.max()) == sum(lengths) - 1
