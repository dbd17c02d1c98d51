"""Fused segmentation masks and localisation from relevancy maps
(langsplatv2_amd.segment, csrc/query_post.hip) against the reference's
post-process of get_max_across_quick's output: eval_lerf.py:111-156
(segmentation_process_cuda), :158-200 (localization_process_cuda), :104-109
(smooth_cuda) and eval_3d_ovs.py:253-258 (the masked-mean level score).

tests/golden/ref_segment.npz holds what the reference's own two functions give
on a seeded (3, 3, 24, 40) fixture in float64 on the CPU
(make_ref_segment.py: eval_lerf imported with stand-ins for the modules absent
here); `ref_post` below is this file's numpy-float64 restatement, pinned to it
(blended maps within 1e-12, IoUs, levels and acc_num equal) and used for every
other shape.

Tolerances (derived from the kernel's summation order, not fitted), with
u = 2^-24 and inputs in [0, 1]: at the reference's 29 taps k_post_smooth sums a
row window as a fixed tree (window29: pairs, fours, eights, then
16 + 8 + 4 + 1 — a tap passes through at most 7 rounded additions; the zeros
staged outside the image add exactly), then a column window of 29 row sums by
the same tree (7 more), then divides by the tap count (1 rounding): every tap
enters the result with a relative error <= (1 + u)^15 - 1 < 15.001 u, and
avg <= 1, so

    AVG_ATOL   = 16 u = 9.54e-7     (the project's REL_ATOL = 5e-6 holds it)

(the other kernel sizes add a window in order, 2 (kernel - 1) + 1 roundings:
test_other_kernel_sizes).  blend = 0.5 * (avg + v): the addition rounds once
(<= u * 2, halved exactly), and the error of avg is halved: 8 u + 1 u = 9 u.
The masked-mean score is a float64 sum of blend rounded to fp32 once and
divided once (2 u more), so

    BLEND_ATOL = 12 u = 7.15e-7

covers both.  A mask pixel may differ from the float64 mask only where the
normalised value o lies within `band` of the threshold, band =
6 BLEND_ATOL / (max - min) + 4 u: the normalisation's amplification of a
BLEND_ATOL error in the value, the minimum and the maximum, plus its own
roundings (a plane with max == min has o = 0 exactly on both sides: the kernel
subtracts the plane's own minimum, so its band is empty).  The seeded cases
keep at most 0.5 % of a plane's pixels inside the band
(test_band_cap_of_seeded_inputs).
Measured on the MI355X over this file's cases: see DESIGN.md, "Fused masks and
localisation".
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from langsplatv2_amd import _lib, segment
from test_query_relevancy import REL_ATOL

U = 2.0 ** -24
AVG_ATOL = 16 * U
BLEND_ATOL = 12 * U
assert BLEND_ATOL <= AVG_ATOL <= REL_ATOL
BAND_CAP = 0.005
THRESH = 0.4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_segment.npz")


# ---------------------------------------------------------------- float64 restatement

def box_sum(a, r):
    """Sum over the (2 r + 1)^2 window clipped to the image, per plane (last two axes)."""
    if r == 0:
        return a.copy()
    H, W = a.shape[-2:]
    p = np.zeros(a.shape[:-2] + (H + 2 * r, W + 2 * r), a.dtype)
    p[..., r:r + H, r:r + W] = a
    rows = np.lib.stride_tricks.sliding_window_view(p, 2 * r + 1, axis=-1).sum(-1)
    return np.lib.stride_tricks.sliding_window_view(rows, 2 * r + 1, axis=-2).sum(-1)


def taps(H, W, r):
    return box_sum(np.ones((H, W), np.int64), r)


def ref_avg(rel, kernel=29):
    r = (kernel - 1) // 2
    return box_sum(rel.astype(np.float64), r) / taps(*rel.shape[-2:], r)


def majority(raw, smooth_kernel=7):
    """smooth_cuda: AvgPool2d(7, 1, 3, count_include_pad=False)(raw) > 0.5, in integers."""
    s = (smooth_kernel - 1) // 2
    return (2 * box_sum(raw.astype(np.int64), s) > taps(*raw.shape[-2:], s)).astype(np.uint8)


def ref_post(rel, thresh=THRESH, kernel=29, smooth_kernel=7, gt=None):
    """The reference's post-process of (L, Q, H, W) maps in numpy float64, from the fp32 input."""
    v = rel.astype(np.float64)
    L, Q, H, W = v.shape
    avg = ref_avg(rel, kernel)
    blend = 0.5 * (avg + v)
    mn, mx = blend.min((-2, -1), keepdims=True), blend.max((-2, -1), keepdims=True)
    out = blend - mn
    out = out / (out.max((-2, -1), keepdims=True) + 1e-9)
    o = np.clip(out * 2.0 - 1.0, 0, 1)
    mask = majority(o > thresh, smooth_kernel)
    area = mask.sum((-2, -1), dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (blend * mask).sum((-2, -1)) / area
    mean[0] = 0.0
    amax = avg.max((-2, -1))
    first = (avg == amax[..., None, None]).reshape(L, Q, -1).argmax(-1)
    r = dict(avg=avg, blend=blend, o=o, mask=mask, area=area, range=(mx - mn)[..., 0, 0], score_max=mx[..., 0, 0],
             score_mean=mean, loc_score=amax, yx=np.stack((first // W, first % W), -1),
             ties=(avg == amax[..., None, None]).sum((-2, -1)))
    if gt is not None:
        g = gt.astype(bool)[None]
        r["inter"] = (mask.astype(bool) & g).sum((-2, -1), dtype=np.int64)
        r["union"] = (mask.astype(bool) | g).sum((-2, -1), dtype=np.int64)
    return r


def band_pixels(ref, thresh=THRESH):
    """Pixels whose float64 normalised value is within the band of the threshold."""
    rng = ref["range"][..., None, None]
    with np.errstate(divide="ignore"):
        band = np.where(rng > 0, 6 * BLEND_ATOL / rng + 4 * U, 0.0)
    return (np.abs(ref["o"] - thresh) <= band) & (rng > 0)


def near_band(ref, smooth_kernel=7, thresh=THRESH):
    """The smooth_kernel^2 neighbourhoods of the band pixels: where a mask may differ."""
    return box_sum(band_pixels(ref, thresh).astype(np.int64), (smooth_kernel - 1) // 2) > 0


def ref_hits(yx, boxes):
    acc = 0
    for (y, x), bs in zip(yx, boxes):
        for x1, y1, x2, y2 in np.asarray(bs).reshape(-1, 4):
            if min(x1, x2) <= x <= max(x1, x2) and min(y1, y2) <= y <= max(y1, y2):
                acc += 1
                break
    return acc


# ---------------------------------------------------------------- seeded inputs

def gauss_blur(a, sigma):
    r = max(1, int(3 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for ax in (-1, -2):
        pad = [(0, 0)] * a.ndim
        pad[ax] = (r, r)
        a = (np.lib.stride_tricks.sliding_window_view(np.pad(a, pad, mode="wrap"), 2 * r + 1, axis=ax) * k).sum(-1)
    return a


def field(g, L, Q, H, W):
    """Relevancy-like planes in (0, 1): a sigmoid of Gaussian-filtered noise plus a little white noise."""
    ch, cw = max(H, 32), max(W, 32)
    z = gauss_blur(g.standard_normal((L, Q, ch, cw)), min(ch, cw) / 10.0)
    z = 3.0 * z / z.std(axis=(-2, -1), keepdims=True)
    v = 0.96 / (1.0 + np.exp(-z)) + 0.02 + 0.02 * (g.random(z.shape) - 0.5)
    return np.ascontiguousarray(v[..., :H, :W]).astype(np.float32)


def gt_for(g, rel):
    """One annotation mask per prompt: a rectangle around level 0's hottest pixel; the last prompt's is empty."""
    L, Q, H, W = rel.shape
    gt = np.zeros((Q, H, W), np.uint8)
    for q in range(Q - 1 if Q > 1 else Q):
        y, x = np.unravel_index(np.argmax(rel[0, q]), (H, W))
        gt[q, max(0, y - H // 4):y + H // 4 + 1, max(0, x - W // 4):x + W // 4 + 1] = 1 + q   # any non-zero = inside
    return gt


SHAPES = [(1, 1), (20, 33), (29, 29), (61, 83), (96, 160)]   # a pixel; every window clipped; the kernel's size;
                                                             # odd, 2 x 2 tiles; 3 x 3 tiles of 32 x 64
STACKS = [(3, 1), (3, 5), (1, 2)]
CASES = [(H, W, L, Q) for (H, W) in SHAPES for (L, Q) in STACKS]


@functools.lru_cache(maxsize=None)
def case(H, W, L, Q):
    """Seeded input, annotation masks and the float64 reference of one shape, shared by the tests (read only)."""
    g = np.random.default_rng(H * 100000 + W * 100 + L * 10 + Q)
    rel = field(g, L, Q, H, W)
    gt = gt_for(g, rel)
    out = dict(rel=rel, gt=gt, **ref_post(rel, gt=gt))
    for v in out.values():
        v.setflags(write=False)
    return out


def to_gpu(a, gpu):
    return torch.tensor(np.asarray(a)).to(gpu)   # (a copy: the shared cases are read-only)


def npy(t):
    return t.detach().cpu().numpy()


def check(got, ref, atol, name):
    got = npy(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == np.float32, name
    assert np.isfinite(got).all(), name
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{name}: max abs err {err:.3e} (bound {atol:.3e})")
    assert err <= atol, f"{name}: max abs err {err:.3e} > {atol:.3e}"


def np_counts(mask, gt):
    m, g = mask.astype(bool), gt.astype(bool)[None]
    return m.sum((-2, -1), dtype=np.int64), (m & g).sum((-2, -1), dtype=np.int64), (m | g).sum((-2, -1),
                                                                                              dtype=np.int64)


# ---------------------------------------------------------------- CPU

def test_restatement_matches_reference_golden():
    z = np.load(GOLDEN)
    rel, gt, boxes = z["rel"], z["gt_masks"], z["boxes"]
    assert rel.shape == (3, 3, 24, 40) and rel.dtype == np.float32 and float(z["thresh"]) == THRESH
    r = ref_post(rel, gt=gt)
    assert np.abs(r["blend"] - z["blended"]).max() <= 1e-12
    # eval_lerf.py:141-151: the IoU is an int64 / int64 true division (fp32), the level the arg-max of the blend's maximum
    lvl = r["score_max"].argmax(0)
    assert np.array_equal(lvl, z["chosen_lvl_list"])
    q = np.arange(3)
    with np.errstate(invalid="ignore"):
        iou = np.float32(r["inter"][lvl, q]) / np.float32(r["union"][lvl, q])
    assert np.array_equal(iou, z["chosen_iou_list"].astype(np.float32))
    assert (r["ties"] == 1).all()
    loc_lvl = r["loc_score"].argmax(0)
    assert ref_hits(r["yx"][loc_lvl, q], boxes) == int(z["acc_num"])
    assert 0 < int(z["acc_num"]) < 3 and len(set(z["chosen_lvl_list"].tolist())) > 1   # the fixture discriminates


def test_restatement_matches_torch_pools():
    """The box mean and the majority are AvgPool2d(count_include_pad=False) in float64."""
    c = case(20, 33, 3, 1)
    t = torch.from_numpy(c["rel"].astype(np.float64))[:, 0:1]
    pool = torch.nn.AvgPool2d(29, stride=1, padding=14, count_include_pad=False)
    assert np.abs(pool(t).numpy()[:, 0] - c["avg"][:, 0]).max() <= 1e-14
    raw = torch.from_numpy((c["o"] > THRESH).astype(np.float32))
    pool7 = torch.nn.AvgPool2d(7, stride=1, padding=3, count_include_pad=False)
    assert np.array_equal((pool7(raw) > 0.5).numpy().astype(np.uint8), c["mask"])


@pytest.mark.parametrize("H,W,L,Q", CASES)
def test_band_cap_of_seeded_inputs(H, W, L, Q):
    """A condition on the inputs: at most 0.5 % of a plane's pixels within the band of the threshold."""
    c = case(H, W, L, Q)
    assert 0.0 < c["rel"].min() and c["rel"].max() < 1.0
    share = band_pixels(c).mean((-2, -1))
    assert share.max() <= BAND_CAP, share


def test_validation_on_cpu():
    rel = torch.zeros(3, 2, 8, 8)
    for f in (segment.smooth_maps, segment.segment_maps, segment.localize_maps):
        with pytest.raises(ValueError):
            f(torch.zeros(2, 8, 8))                                        # rank
        with pytest.raises(ValueError):
            f(rel.double())                                                # dtype
        with pytest.raises(ValueError):
            f(rel.permute(0, 1, 3, 2))                                     # not contiguous
        with pytest.raises(ValueError):
            f(torch.zeros(3, 0, 8, 8))                                     # empty
        with pytest.raises(ValueError):
            f(rel, kernel=28)                                              # even
        with pytest.raises(ValueError):
            f(rel, kernel=65)                                              # out of range
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(rel)
    with pytest.raises(ValueError):
        segment.segment_maps(rel, smooth_kernel=6)
    with pytest.raises(ValueError):
        segment.segment_maps(rel, smooth_kernel=17)
    with pytest.raises(ValueError):
        segment.segment_maps(rel, select="mean")
    with pytest.raises(ValueError):
        segment.segment_maps(rel, gt_masks=torch.zeros(3, 8, 8, dtype=torch.uint8))    # (Q, H, W) wanted
    with pytest.raises(ValueError):
        segment.segment_maps(rel, gt_masks=torch.zeros(2, 8, 8))                       # dtype
    with pytest.raises(RuntimeError, match="no CPU path"):
        segment.segment_maps(rel, gt_masks=torch.zeros(2, 8, 8, dtype=torch.uint8))


def test_abi_status_codes_without_device():
    lib = _lib.load()
    f = ctypes.c_float
    ws = lib.lsr_query_post_workspace_bytes
    assert ws(12, 1080, 1920) > 0 and ws(1, 1, 1) > 0
    assert ws(0, 8, 8) == 0 and ws(70000, 8, 8) == 0 and ws(1, 65536, 65536) == 0 and ws(-1, 8, 8) == 0
    sm = lib.lsr_query_smooth
    assert sm(None, 1, 8, 8, 29, None, None, None, None, None, None) == 1                    # null input
    assert sm(1, 1, 8, 8, 29, None, None, None, 1, 1, None) == 1                             # null stats
    assert sm(1, 1, 8, 8, 28, None, None, 1, 1, 1, None) == 1                                # even kernel
    assert sm(1, 1, 8, 8, 0, None, None, 1, 1, 1, None) == 1
    assert sm(1, 1, 8, 8, 65, None, None, 1, 1, 1, None) == 2                                # kernel out of range
    assert sm(1, 70000, 8, 8, 29, None, None, 1, 1, 1, None) == 2                            # shape out of range
    for planes, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert sm(None, planes, H, W, 29, None, None, None, None, None, None) == 0           # nothing to do
    mk = lib.lsr_query_mask
    assert mk(None, None, None, 2, 1, 8, 8, f(0.4), 7, None, None, None, None, None) == 1    # null input
    assert mk(1, 1, None, 2, 1, 8, 8, f(0.4), 7, None, 1, 1, 1, None) == 1                   # null mask
    assert mk(1, 1, None, 2, 1, 8, 8, f(0.4), 6, 1, 1, 1, 1, None) == 1                      # even kernel
    assert mk(1, 1, 1, 3, 2, 8, 8, f(0.4), 7, 1, 1, 1, 1, None) == 1                         # planes % n_prompt
    assert mk(1, 1, None, 2, 1, 8, 8, f(0.4), 17, 1, 1, 1, 1, None) == 2                     # kernel out of range
    for planes, H, W in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert mk(None, None, None, planes, 1, H, W, f(0.4), 7, None, None, None, None, None) == 0


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("H,W,L,Q", CASES)
def test_avg_and_blend_match_float64(gpu, H, W, L, Q):
    c = case(H, W, L, Q)
    rel = to_gpu(c["rel"], gpu)
    avg, blend = segment.smooth_maps(rel)
    check(avg, c["avg"], AVG_ATOL, f"avg {L}x{Q}x{H}x{W}")
    check(blend, c["blend"], BLEND_ATOL, f"blend {L}x{Q}x{H}x{W}")
    only_avg, none = segment.smooth_maps(rel, want_blend=False)
    assert none is None and torch.equal(only_avg, avg)
    none, only_blend = segment.smooth_maps(rel, want_avg=False)
    assert none is None and torch.equal(only_blend, blend)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [1, 3, 15, 17, 63])
def test_other_kernel_sizes(gpu, kernel):
    """kernel = 1 returns the input bit for bit; the run-time-radius kernels
    (both LDS sizes) add a window's terms in order: (kernel - 1) roundings along
    the row, as many down the column and the division, < 2 kernel u."""
    c = case(61, 83, 3, 1)
    rel = to_gpu(c["rel"], gpu)
    avg, blend = segment.smooth_maps(rel, kernel=kernel)
    if kernel == 1:
        assert torch.equal(avg, rel) and torch.equal(blend, rel)
        return
    ref = ref_avg(c["rel"], kernel)
    atol = 2 * kernel * U
    check(avg, ref, atol, f"avg kernel {kernel}")
    check(blend, 0.5 * (ref + c["rel"]), 0.5 * atol + U, f"blend kernel {kernel}")


@pytest.mark.gpu
def test_constant_plane(gpu):
    H, W = 45, 70
    rel = torch.full((2, 2, H, W), 0.5, device=gpu)
    avg, blend = segment.smooth_maps(rel)
    assert torch.all(avg == 0.5) and torch.all(blend == 0.5)
    gt = torch.zeros(2, H, W, dtype=torch.uint8, device=gpu)
    gt[0, 3:9, 5:20] = 1                                                   # prompt 0 annotated, prompt 1 empty
    s = segment.segment_maps(rel, gt_masks=gt)
    assert not s.masks.any() and not s.area.any() and torch.all(s.score == 0.5)
    assert torch.all(s.inter == 0) and torch.equal(s.union, torch.tensor([[90, 0], [90, 0]], device=gpu))
    assert torch.all(s.iou[:, 0] == 0) and torch.isnan(s.iou[:, 1]).all()
    loc = segment.localize_maps(rel)
    assert torch.all(loc.score == 0.5) and not loc.yx.any() and torch.all(loc.ties == H * W)
    assert not loc.yx_chosen.any() and not loc.level.any()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,L,Q", CASES)
def test_masks_and_counts(gpu, H, W, L, Q):
    c = case(H, W, L, Q)
    rel, gt = to_gpu(c["rel"], gpu), to_gpu(c["gt"], gpu)
    s = segment.segment_maps(rel, THRESH, gt_masks=gt)
    m = npy(s.masks)
    assert m.dtype == np.uint8 and m.shape == (L, Q, H, W) and m.max() <= 1
    free = ~near_band(c)
    print(f"masks {L}x{Q}x{H}x{W}: {int((m != c['mask']).sum())} pixels differ, {int((~free).sum())} near the band")
    assert np.array_equal(m[free], c["mask"][free])
    area, inter, union = np_counts(m, c["gt"])
    assert np.array_equal(npy(s.area), area) and np.array_equal(npy(s.inter), inter)
    assert np.array_equal(npy(s.union), union)
    assert s.area.dtype == s.inter.dtype == s.union.dtype == torch.int64
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(npy(s.iou), inter.astype(np.float32) / union.astype(np.float32))
    raw = segment.segment_maps(rel, THRESH, smooth_kernel=1)
    assert raw.inter is None and raw.union is None and raw.iou is None
    assert np.array_equal(m, majority(npy(raw.masks)))
    assert torch.equal(raw.blend, s.blend)
    # a bool annotation mask is read as it is
    assert torch.equal(segment.segment_maps(rel, THRESH, gt_masks=gt != 0).inter, s.inter)


@pytest.mark.gpu
@pytest.mark.parametrize("smooth_kernel", [3, 9, 15])
def test_other_majority_sizes(gpu, smooth_kernel):
    c = case(61, 83, 3, 1)
    rel = to_gpu(c["rel"], gpu)
    raw = segment.segment_maps(rel, THRESH, smooth_kernel=1)
    got = segment.segment_maps(rel, THRESH, smooth_kernel=smooth_kernel)
    assert np.array_equal(npy(got.masks), majority(npy(raw.masks), smooth_kernel))


@pytest.mark.gpu
def test_threshold_extremes(gpu):
    c = case(61, 83, 3, 1)
    rel = to_gpu(c["rel"], gpu)
    ones = segment.segment_maps(rel, -1.0)
    assert torch.all(ones.masks == 1) and torch.all(ones.area == 61 * 83)
    zeros = segment.segment_maps(rel, 1.0)
    assert not zeros.masks.any() and not zeros.area.any()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,L,Q", CASES)
def test_scores_and_levels(gpu, H, W, L, Q):
    c = case(H, W, L, Q)
    rel = to_gpu(c["rel"], gpu)
    s = segment.segment_maps(rel, THRESH)
    check(s.score, c["score_max"], BLEND_ATOL, f"max score {L}x{Q}x{H}x{W}")
    assert torch.equal(s.score, s.blend.amax((-2, -1)))
    sm = segment.segment_maps(rel, THRESH, select="masked_mean")
    assert torch.equal(sm.masks, s.masks) and torch.all(sm.score[0] == 0)
    same = (npy(sm.masks) == c["mask"]).all((-2, -1))
    got, ref = npy(sm.score).astype(np.float64), c["score_mean"]
    assert np.array_equal(np.isnan(got[same]), np.isnan(ref[same]))
    ok = same & ~np.isnan(ref)
    err = float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
    print(f"masked mean {L}x{Q}x{H}x{W}: max abs err {err:.3e} over {int(ok.sum())} planes (bound {BLEND_ATOL:.3e})")
    assert err <= BLEND_ATOL
    for res, ref_score, every in ((s, c["score_max"], True), (sm, c["score_mean"], bool(same.all()))):
        assert res.level.dtype == torch.int64 and res.level.shape == (Q,)
        assert torch.equal(res.level, res.score.argmax(0))
        if L > 1 and every and not np.isnan(ref_score).any():
            top = np.sort(ref_score, axis=0)
            clear = top[-1] - top[-2] > 2 * BLEND_ATOL
            assert np.array_equal(npy(res.level)[clear], ref_score.argmax(0)[clear])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,L,Q", CASES)
def test_localisation(gpu, H, W, L, Q):
    c = case(H, W, L, Q)
    loc = segment.localize_maps(to_gpu(c["rel"], gpu))
    check(loc.score, c["loc_score"], AVG_ATOL, f"localisation score {L}x{Q}x{H}x{W}")
    yx = npy(loc.yx)
    assert yx.dtype == np.int64 and yx.shape == (L, Q, 2)
    assert (yx >= 0).all() and (yx[..., 0] < H).all() and (yx[..., 1] < W).all()
    at = np.take_along_axis(c["avg"].reshape(L, Q, -1), (yx[..., 0] * W + yx[..., 1])[..., None], -1)[..., 0]
    assert (c["loc_score"] - at).max() <= 2 * AVG_ATOL
    assert (npy(loc.ties) >= 1).all()
    assert torch.equal(loc.level, loc.score.argmax(0))
    assert torch.equal(loc.yx_chosen, loc.yx[loc.level, torch.arange(Q, device=gpu)])
    # the maximum, its first pixel and the tie count are those of the kernel's own avg
    avg, _ = segment.smooth_maps(to_gpu(c["rel"], gpu), want_blend=False)
    flat = avg.reshape(L, Q, -1)
    assert torch.equal(loc.score, flat.amax(-1))
    hit = flat == loc.score[..., None]
    assert torch.equal(loc.ties, hit.sum(-1))
    assert torch.equal(loc.yx[..., 0] * W + loc.yx[..., 1], hit.int().argmax(-1))


@pytest.mark.gpu
def test_two_equal_plateaus(gpu):
    """Two planted 31 x 31 blocks of 0.75 on zeros: the box mean is 0.75 exactly
    on each block's central 3 x 3 pixels (630.75 / 841), in different tiles; the
    first in row-major order is returned and the tie count covers both."""
    H, W = 72, 110
    rel = torch.zeros(1, 2, H, W, device=gpu)
    rel[0, 0, 5:36, 8:39] = 0.75
    rel[0, 0, 38:69, 70:101] = 0.75
    rel[0, 1, 38:69, 70:101] = 0.75                                        # the second plateau alone
    loc = segment.localize_maps(rel)
    assert torch.all(loc.score == 0.75)
    assert npy(loc.yx).tolist() == [[[19, 22], [52, 84]]]
    assert npy(loc.ties).tolist() == [[18, 9]]
    assert segment.hits(loc, [[[0, 0, 5, 5], [30, 25, 20, 15]], [[84, 52, 84, 52]]]) == 2
    assert segment.hits(loc, [[[23, 19, 40, 40]], [[85, 52, 90, 60]]]) == 0


@pytest.mark.gpu
def test_reproducible_stream_and_input_untouched(gpu):
    c = case(96, 160, 3, 5)
    rel, gt = to_gpu(c["rel"], gpu), to_gpu(c["gt"], gpu)
    keep = rel.clone()

    def run():
        s = segment.segment_maps(rel, THRESH, gt_masks=gt, select="masked_mean")
        return list(s) + list(segment.localize_maps(rel)) + list(segment.smooth_maps(rel))

    def same(a, b):
        return all(torch.equal(x, y) if not x.is_floating_point() else
                   torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))

    first = run()
    second = run()
    torch.cuda.synchronize()
    assert same(first, second)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        third = run()
        sums = torch.stack([t.double().sum() for t in third[:2]])          # used on the caller's stream, no sync
    torch.cuda.synchronize()
    assert same(first, third)
    assert torch.equal(sums, torch.stack([t.double().sum() for t in first[:2]]))
    assert torch.equal(rel, keep)


@pytest.mark.gpu
def test_golden(gpu):
    z = np.load(GOLDEN)
    rel, gt = to_gpu(z["rel"], gpu), to_gpu(z["gt_masks"], gpu)
    r = ref_post(z["rel"], gt=z["gt_masks"])
    s = segment.segment_maps(rel, float(z["thresh"]), gt_masks=gt)
    check(s.blend, z["blended"], BLEND_ATOL, "golden blended maps")
    assert npy(s.level).tolist() == z["chosen_lvl_list"].tolist()
    # IoU by the band rule: the counts may move by at most the pixels near the band (none: equal)
    slack = near_band(r).sum((-2, -1))
    print("golden: pixels near the band per plane", slack.tolist())
    assert (np.abs(npy(s.inter) - r["inter"]) <= slack).all() and (np.abs(npy(s.union) - r["union"]) <= slack).all()
    q = np.arange(3)
    lvl = z["chosen_lvl_list"]
    if not slack[lvl, q].any():
        assert np.array_equal(npy(s.iou)[lvl, q], z["chosen_iou_list"].astype(np.float32))
    loc = segment.localize_maps(rel)
    assert segment.hits(loc, z["boxes"]) == int(z["acc_num"])


@pytest.mark.gpu
def test_render_then_segment_end_to_end(gpu, oracle_lib):
    """Quick render -> relevancy_maps -> segment_maps / localize_maps, vs the
    restatement applied to the GPU's own fp32 relevancy."""
    from harness import make_case
    from langsplatv2_amd import query
    from test_query_relevancy import unit
    from test_quick_stream import _renderer
    case_ = make_case(N=3000, W=96, H=80, seed=21, sh_degree=None, quick_k=4)
    wm = _renderer(case_, gpu, None)()
    g = np.random.default_rng(3)
    cb, pos, neg = g.standard_normal((3, 64, 512)).astype(np.float32), unit(g, 3), unit(g, 4)
    rel = query.relevancy_maps(wm, *(to_gpu(a, gpu) for a in (cb, pos, neg)))
    assert rel.shape == (3, 3, 80, 96)
    gt = np.zeros((3, 80, 96), np.uint8)
    gt[:, 20:60, 30:70] = 1
    r = ref_post(npy(rel), gt=gt)
    s = segment.segment_maps(rel, THRESH, gt_masks=to_gpu(gt, gpu))
    check(s.blend, r["blend"], BLEND_ATOL, "render + relevancy + blend")
    free = ~near_band(r)
    m = npy(s.masks)
    print(f"end to end: {int((m != r['mask']).sum())} mask pixels differ, {int((~free).sum())} near the band")
    assert np.array_equal(m[free], r["mask"][free])
    area, inter, union = np_counts(m, gt)
    assert np.array_equal(npy(s.area), area) and np.array_equal(npy(s.inter), inter)
    assert np.array_equal(npy(s.union), union)
    check(s.score, r["score_max"], BLEND_ATOL, "render + relevancy + score")
    loc = segment.localize_maps(rel)
    check(loc.score, r["loc_score"], AVG_ATOL, "render + relevancy + localisation score")
    yx = npy(loc.yx)
    at = r["avg"][np.arange(3)[:, None], np.arange(3)[None], yx[..., 0], yx[..., 1]]
    assert (r["loc_score"] - at).max() <= 2 * AVG_ATOL
