"""langsplatv2_amd/mask_nms.py: SAM mask NMS and segment maps of the preprocess
step (csrc/mask_nms.hip, C ABI lsr_mask_*), replacing mask_nms / masks_update
(preprocess.py:215-294) and mask2segmap with create's offsets (:304-317, :145-157).

Every comparison is exact; there is no tolerance.  The chain of evidence:

  reference's own mask_nms (run on the CPU by tests/golden/make_ref_mask_nms.py)
      == tests/golden/ref_mask_nms.npz
      == `restate` below (vectorised float32 torch, intersections by integer matmul)   [CPU tests]
      == the HIP path, on the fixture and on cases the reference cannot run            [GPU tests]

The reference raises IndexError in its three "top 3" fallbacks, so those are
pinned by `restate` alone, which implements what the reference's comment states.

The inner-l fallback needs l_max to fail in every column.  With a threshold
1 - inner_thr >= 0 that cannot happen: the column of a mask of largest area
would need a partner r with I / A_r < 0.5 and I >= 0.85 A_max, so A_r > A_max.
So the built case uses inner_thr = 1.5 (threshold -0.5): every l_max and every
u_max, both >= 0, fail, and both inner fallbacks fire.
"""
import ctypes
import functools
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch

from langsplatv2_amd import _lib

# the package also exports the function mask_nms under the module's name
MN = importlib.import_module("langsplatv2_amd.mask_nms")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ref_mask_nms.npz")
SITE = dict(iou_thr=0.8, score_thr=0.7, inner_thr=0.5)   # preprocess.py:302
DEFAULTS = dict(iou_thr=0.7, score_thr=0.1, inner_thr=0.2)


@functools.lru_cache(maxsize=None)
def maker():
    spec = importlib.util.spec_from_file_location("make_ref_mask_nms", os.path.join(HERE, "golden", "make_ref_mask_nms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    """name -> (masks (N, H, W) bool, scores float64, selected int64); shared, never modified."""
    z = np.load(GOLD)
    out = {}
    for name in z["cases"]:
        name = str(name)
        N, H, W = (int(v) for v in z[name + "_shape"])
        masks = np.unpackbits(z[name + "_bits"], axis=1, bitorder="little")[:, :H * W].reshape(N, H, W).astype(bool)
        out[name] = (masks, z[name + "_scores"], z[name + "_selected"])
    assert tuple(z["thresholds"]) == (SITE["iou_thr"], SITE["score_thr"], SITE["inner_thr"])
    return out


FIXTURE_NAMES = sorted(str(n) for n in np.load(GOLD)["cases"])


def restate(masks, scores, iou_thr=0.7, score_thr=0.1, inner_thr=0.2, tril_diagonal=1):
    """preprocess.py:230-279 vectorised, float32, on the CPU.  masks (N, H, W) bool
    array, scores a torch vector (its dtype kept).  Returns selected_idx and the
    four per-rank keep vectors (iou, conf, inner_u, inner_l) after the fallbacks.
    tril_diagonal=0 leaves out the superdiagonal the reference's tril keeps."""
    ranked, idx = torch.sort(scores, dim=0, descending=True, stable=True)
    m = torch.from_numpy(np.ascontiguousarray(masks))[idx].flatten(1).to(torch.int64)
    N = m.shape[0]
    inter = m @ m.T
    area = inter.diagonal()
    I = inter.float()
    iou = I / (area[:, None] + area[None, :] - inter).float()
    a = I / area.float()[:, None]          # over the higher-scoring mask's area
    b = I / area.float()[None, :]          # over the lower-scoring mask's area
    inner = 1 - b * a
    upper = torch.ones(N, N, dtype=torch.bool).triu(1)
    zero = torch.zeros((), dtype=torch.float32)
    U = torch.where(upper & (a < 0.5) & (b >= 0.85), inner, zero)
    L = torch.where(upper & (a >= 0.85) & (b < 0.5), inner, zero).T    # row j, column i
    mat = U + L
    iou_max = torch.triu(iou, 1).max(dim=0).values
    u_max = torch.triu(mat, 1).max(dim=0).values
    l_max = torch.tril(mat, tril_diagonal).max(dim=0).values
    k_iou = iou_max <= iou_thr
    k_conf = ranked > score_thr
    k_u = u_max <= 1 - inner_thr
    k_l = l_max <= 1 - inner_thr
    for k in (k_conf, k_u, k_l):   # what the reference's comment states; its code raises IndexError
        if k.sum() == 0:
            k[:3] = True
    return idx[k_iou & k_conf & k_u & k_l], (k_iou, k_conf, k_u, k_l)


def np_words(masks):
    """(N, ceil(H W / 64)) int64 words and (N,) areas from numpy.packbits."""
    N = masks.shape[0]
    flat = masks.reshape(N, -1) != 0
    by = np.packbits(flat, axis=1, bitorder="little")
    pad = (-by.shape[1]) % 8
    by = np.concatenate([by, np.zeros((N, pad), dtype=np.uint8)], axis=1)
    return np.ascontiguousarray(by).view("<u8").astype(np.int64), flat.sum(1).astype(np.int32)


def random_masks(N, H, W, seed, p=0.3):
    return np.random.RandomState(seed).random_sample((N, H, W)) < p


def matmul_table(masks):
    m = masks.reshape(masks.shape[0], -1).astype(np.int64)
    return np.triu(m @ m.T).astype(np.int32)


# ------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_restatement_equals_reference(name):
    masks, scores, selected = fixture()[name]
    got, _ = restate(masks, torch.from_numpy(scores), **SITE)
    assert got.dtype == torch.int64
    assert got.tolist() == selected.tolist()


def test_fixture_exercises_every_criterion_alone():
    alone = [0, 0, 0, 0]
    superdiag = 0
    for name in FIXTURE_NAMES:
        masks, scores, _ = fixture()[name]
        _, ks = restate(masks, torch.from_numpy(scores), **SITE)
        _, ks0 = restate(masks, torch.from_numpy(scores), tril_diagonal=0, **SITE)
        for c in range(4):
            others = torch.stack([ks[o] for o in range(4) if o != c]).all(0)
            alone[c] += int((~ks[c] & others).sum())
        superdiag += int((~ks[3] & ks0[3]).sum())   # dropped by inner_l only because tril keeps the superdiagonal
    print("dropped by iou / conf / inner_u / inner_l alone:", alone, "; inner_l drops due to the superdiagonal:", superdiag)
    assert all(n >= 1 for n in alone), alone
    assert superdiag >= 1


def test_c_abi_argument_checks():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 1024)()
    P = (ctypes.addressof(buf) + 255) & ~255   # a 256-B aligned stand-in address, never dereferenced
    OK, EINVAL, EUNSUPPORTED = 0, 1, 2
    wsb = lib.lsr_mask_nms_workspace_bytes
    assert wsb(1) >= 4 and wsb(4096) >= 4 * 4096 * 4096 and wsb(0) > 0
    assert wsb(-1) == 0 and wsb(4097) == 0
    big_h, big_w = 4096, 4097   # H W = 2^24 + 4096
    for args, want in [                      # lsr_mask_pack(masks, N, H, W, words, area, stream)
            ((None, 5, 3, 5, P, P, None), EINVAL), ((P, 5, 3, 5, None, P, None), EINVAL),
            ((P, 5, 3, 5, P, None, None), EINVAL), ((P, 5, 3, 5, P + 4, P, None), EINVAL),
            ((P, -1, 3, 5, P, P, None), EINVAL), ((P, 5, 0, 5, P, P, None), EINVAL),
            ((P, 5, 3, 0, P, P, None), EINVAL), ((P, 4097, 3, 5, P, P, None), EUNSUPPORTED),
            ((P, 5, big_h, big_w, P, P, None), EUNSUPPORTED), ((None, 0, 0, 5, None, None, None), EINVAL),
            ((None, 0, 3, 5, None, None, None), OK)]:
        assert lib.lsr_mask_pack(*args) == want, args
    for args, want in [                      # lsr_mask_pair_counts(words, N, H, W, order, inter, stream)
            ((None, 5, 3, 5, None, P, None), EINVAL), ((P, 5, 3, 5, None, None, None), EINVAL),
            ((P + 4, 5, 3, 5, None, P, None), EINVAL), ((P, -1, 3, 5, None, P, None), EINVAL),
            ((P, 4097, 3, 5, None, P, None), EUNSUPPORTED), ((P, 5, big_h, big_w, None, P, None), EUNSUPPORTED),
            ((None, 0, 3, 5, None, None, None), OK)]:
        assert lib.lsr_mask_pair_counts(*args) == want, args
    # lsr_mask_nms_select(words, area, N, H, W, order, conf, iou_thr, inner_thr, workspace, keep, criteria,
    #                     selected, count, stream)
    good = [P, P, 5, 3, 5, P, P, 0.8, 0.5, P, P, None, P, P, None]
    for pos in (0, 1, 5, 6, 9, 10, 12, 13):      # each required pointer
        args = list(good)
        args[pos] = None
        assert lib.lsr_mask_nms_select(*args) == EINVAL, pos
    for pos, val, want in [(9, P + 4, EINVAL), (2, -1, EINVAL), (2, 4097, EUNSUPPORTED), (3, 0, EINVAL)]:
        args = list(good)
        args[pos] = val
        assert lib.lsr_mask_nms_select(*args) == want, (pos, val)
    args = list(good)
    args[3], args[4] = big_h, big_w
    assert lib.lsr_mask_nms_select(*args) == EUNSUPPORTED
    assert lib.lsr_mask_nms_select(None, None, 0, 3, 5, None, None, 0.8, 0.5, None, None, None, None, None, None) == OK
    # lsr_mask_segmaps(words[4], kept[4], masks[4], counts[4], offsets[4], H, W, index_type, out, stream)
    p4, i4 = ctypes.c_void_p * 4, ctypes.c_int32 * 4
    seg = lib.lsr_mask_segmaps
    assert seg(None, p4(), i4(), i4(), i4(), 3, 5, 0, P, None) == EINVAL
    assert seg(p4(), p4(), i4(), i4(), i4(), 3, 5, 0, None, None) == EINVAL
    assert seg(p4(), p4(), i4(), i4(), i4(), 3, 5, 2, P, None) == EINVAL            # int64 maps are not offered
    assert seg(p4(), p4(), i4(), i4(), i4(), 0, 5, 0, P, None) == EINVAL
    assert seg(p4(), p4(), i4(), i4(), i4(), big_h, big_w, 0, P, None) == EUNSUPPORTED
    assert seg(p4(), p4(), i4(2), i4(1), i4(), 3, 5, 0, P, None) == EINVAL          # a counted level without pointers
    assert seg(p4(P), p4(P), i4(2), i4(-1), i4(), 3, 5, 0, P, None) == EINVAL
    assert seg(p4(P), p4(P), i4(2), i4(1), i4(-1), 3, 5, 0, P, None) == EINVAL
    assert seg(p4(P), p4(P), i4(2), i4(4097), i4(), 3, 5, 0, P, None) == EUNSUPPORTED
    assert seg(p4(P), p4(P), i4(4097), i4(1), i4(), 3, 5, 0, P, None) == EUNSUPPORTED


def test_python_argument_errors():
    masks = torch.zeros((3, 4, 5), dtype=torch.bool)
    scores = torch.tensor([0.9, 0.8, 0.7])
    with pytest.raises(RuntimeError, match="no CPU path"):
        MN.pack_masks(masks)
    with pytest.raises(RuntimeError, match="no CPU path"):
        MN.mask_nms(masks, scores)
    with pytest.raises(RuntimeError, match="no CPU path"):
        MN.build_seg_maps([masks])
    cpu_packed = MN.PackedMasks(torch.zeros((3, 1), dtype=torch.int64), torch.zeros(3, dtype=torch.int32), 4, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        MN.mask_pair_counts(cpu_packed)
    with pytest.raises(ValueError, match="3-D"):
        MN.pack_masks(masks[0])
    with pytest.raises(ValueError, match="3-D"):
        MN.mask_nms(masks[0], scores)
    with pytest.raises(ValueError, match="1-D"):
        MN.mask_nms(masks, scores[:, None])
    with pytest.raises(ValueError, match="3 masks but 2 scores"):
        MN.mask_nms(masks, scores[:2])
    with pytest.raises(ValueError, match="floating"):
        MN.mask_nms(masks, torch.tensor([3, 2, 1]))
    with pytest.raises(ValueError, match="dtype"):
        MN.build_seg_maps([masks], dtype=torch.int64)
    with pytest.raises(ValueError, match="levels"):
        MN.build_seg_maps([masks] * 5)
    with pytest.raises(ValueError, match="frame size"):
        MN.build_seg_maps([None, None])


# ------------------------------------------------------------------- GPU ---
def run_nms(gpu, masks, scores, **thr):
    return MN.mask_nms(torch.from_numpy(np.ascontiguousarray(masks)).to(gpu), scores.to(gpu), return_detail=True, **thr)


def check_against_restatement(gpu, masks, scores, what, **thr):
    want, ks = restate(masks, scores, **thr)
    got = run_nms(gpu, masks, scores, **thr)
    crit = got.criteria.cpu()
    for bit, k, nm in zip((MN.CRIT_IOU, MN.CRIT_CONF, MN.CRIT_INNER_U, MN.CRIT_INNER_L), ks,
                          ("iou", "conf", "inner_u", "inner_l")):
        assert ((crit & bit) != 0).tolist() == k.tolist(), (what, nm)
    assert got.keep.cpu().tolist() == torch.stack(ks).all(0).tolist(), what
    assert got.selected.dtype == torch.int64 and got.selected.cpu().tolist() == want.tolist(), what
    return got, ks


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(3, 5), (8, 8), (8, 9), (65, 130), (5, 16), (40, 56), (48, 352)])
def test_pack_matches_packbits(gpu, hw):
    """H W = 15 (under one word), 64, 72 (a full wave and a partial one), 8450; and multiples of
    16, which take the kernel with 16-B loads: 80 (a partial word), 2240 (35 words, a wave step
    is 16) and 16896 (264 words, a workgroup takes 128).  A byte-offset view of a larger buffer
    has no 16-B alignment and takes the byte kernel whatever its size."""
    H, W = hw
    masks = random_masks(5, H, W, seed=H * W, p=0.5)
    masks[1] = True    # a full mask: the tail bits must still be zero
    masks[2] = False
    words, area = np_words(masks)
    as_bool = torch.from_numpy(masks).to(gpu)
    as_u8 = torch.from_numpy(masks.astype(np.uint8) * 3).to(gpu)   # any nonzero byte is set
    wide = torch.zeros((5, H, 2 * W), dtype=torch.uint8, device=gpu)
    wide[:, :, ::2] = as_u8
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    odd = torch.zeros(5 * H * W + 3, dtype=torch.uint8, device=gpu)[3:].view(5, H, W)
    odd.copy_(as_u8)
    assert odd.is_contiguous() and odd.data_ptr() % 16 != 0
    for src in (as_bool, as_u8, view, odd):
        p = MN.pack_masks(src)
        assert (p.H, p.W) == (H, W) and p.words.dtype == torch.int64 and p.area.dtype == torch.int32
        assert np.array_equal(p.words.cpu().numpy(), words)
        assert np.array_equal(p.area.cpu().numpy(), area)
    tail = (-H * W) % 64
    if tail:
        last = MN.pack_masks(as_bool).words[:, -1].cpu().numpy().view(np.uint64)
        assert not (last >> np.uint64(64 - tail)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 33, 64, 65, 97])   # the pair tile is 64 x 64 masks
def test_pair_counts_equal_matmul(gpu, N):
    masks = random_masks(N, 20, 31, seed=N)
    packed = MN.pack_masks(torch.from_numpy(masks).to(gpu))
    got = MN.mask_pair_counts(packed)
    assert got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), matmul_table(masks))
    order = torch.from_numpy(np.random.RandomState(N).permutation(N))
    got = MN.mask_pair_counts(packed, order.to(gpu))
    assert np.array_equal(got.cpu().numpy(), matmul_table(masks[order.numpy()]))


@pytest.mark.gpu
def test_pair_counts_across_word_chunks(gpu):
    """The kernel stages LSR_MASK_WORD_CHUNK = 32 words (2048 pixels) of every mask per
    step and gives a workgroup at least 8 chunks: 8450 pixels are 133 words = 5 chunks (the
    last partial) in one workgroup; 130 x 300 pixels are 610 words = 20 chunks over 2 workgroups."""
    for N, H, W in [(7, 65, 130), (70, 130, 300)]:
        masks = random_masks(N, H, W, seed=H)
        got = MN.mask_pair_counts(MN.pack_masks(torch.from_numpy(masks).to(gpu)))
        assert np.array_equal(got.cpu().numpy(), matmul_table(masks)), (N, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_mask_nms_equals_reference(gpu, name):
    masks, scores, selected = fixture()[name]
    got, _ = check_against_restatement(gpu, masks, torch.from_numpy(scores), name, **SITE)
    assert got.selected.cpu().tolist() == selected.tolist()


def extra_cases():
    """name -> (masks, scores, thresholds): what the reference cannot run or the fixture does not hold."""
    M = maker()
    out = {}
    masks, scores = M.rect_scene(33, 40, 56, 5)
    out["float32_scores"] = (masks, torch.from_numpy(scores).float(), SITE)
    masks, scores = M.rect_scene(97, 48, 70, 6)
    out["default_thresholds"] = (masks, torch.from_numpy(scores), DEFAULTS)
    for N in (2, 5):   # every score below score_thr: ranks 0 .. min(3, N) - 1 count as confident
        masks, scores = M.rect_scene(N, 8, 9, 7)
        out[f"conf_fallback_{N}"] = (masks, torch.from_numpy(scores * 0.5), SITE)
    masks, scores = M.rect_scene(33, 40, 56, 8)    # module docstring: the only way to fail l_max in every column
    out["inner_fallbacks"] = (masks, torch.from_numpy(scores), dict(iou_thr=0.8, score_thr=0.7, inner_thr=1.5))
    masks, scores = M.rect_scene(64, 65, 130, 9)   # four distinct scores: a stable sort keeps input order
    out["tied_scores"] = (masks, torch.from_numpy(np.round(scores * 5) / 5), SITE)
    box = np.zeros((4, 6, 11), dtype=bool)
    box[0, 1:5, 2:9] = True
    box[3, 0:3, 0:4] = True                        # masks 1 and 2 are empty: their pair is 0 / 0
    out["two_empty"] = (box, torch.tensor([0.95, 0.9, 0.85, 0.8], dtype=torch.float64), SITE)
    out["one_empty"] = (box[[0, 1, 3]], torch.tensor([0.95, 0.9, 0.8], dtype=torch.float64), SITE)
    out["single_empty"] = (box[1:2], torch.tensor([0.9], dtype=torch.float64), SITE)
    return out


EXTRA_NAMES = ["float32_scores", "default_thresholds", "conf_fallback_2", "conf_fallback_5", "inner_fallbacks",
               "tied_scores", "two_empty", "one_empty", "single_empty"]


def test_extra_cases_reach_what_they_are_built_for():
    cases = extra_cases()
    assert sorted(cases) == sorted(EXTRA_NAMES)
    for N in (2, 5):
        masks, scores, thr = cases[f"conf_fallback_{N}"]
        assert not bool((scores > thr["score_thr"]).any())
        assert restate(masks, scores, **thr)[1][1].tolist() == [r < 3 for r in range(N)]
    masks, scores, thr = cases["inner_fallbacks"]
    _, ks = restate(masks, scores, **thr)
    assert ks[2].tolist() == ks[3].tolist() == [r < 3 for r in range(33)]
    masks, scores, thr = cases["tied_scores"]
    assert len(set(scores.tolist())) < 8
    sel, ks = restate(*cases["two_empty"][:2], **SITE)
    assert ks[0].tolist() == [True, True, False, True] and sel.tolist() == [0, 1, 3]   # the second empty mask meets NaN
    assert restate(*cases["one_empty"][:2], **SITE)[0].tolist() == [0, 1, 2]
    assert restate(*cases["single_empty"][:2], **SITE)[0].tolist() == [0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXTRA_NAMES)
def test_mask_nms_equals_restatement(gpu, name):
    masks, scores, thr = extra_cases()[name]
    check_against_restatement(gpu, masks, scores, name, **thr)


@pytest.mark.gpu
def test_packed_input_and_batches(gpu):
    masks, scores, selected = fixture()["rect_97x48x70_s0"]
    dm, ds = torch.from_numpy(masks).to(gpu), torch.from_numpy(scores).to(gpu)
    whole = MN.pack_masks(dm)
    joined = MN.PackedMasks.cat([MN.pack_masks(dm[:40]), MN.pack_masks(dm[40:])])
    assert torch.equal(joined.words, whole.words) and torch.equal(joined.area, whole.area)
    assert (joined.H, joined.W) == (whole.H, whole.W) and len(joined) == 97
    assert MN.mask_nms(joined, ds, **SITE).cpu().tolist() == selected.tolist()
    assert MN.mask_nms(dm, ds, **SITE).cpu().tolist() == selected.tolist()
    empty = MN.mask_nms(dm[:0], ds[:0], **SITE)
    assert empty.dtype == torch.int64 and empty.shape == (0,)


@pytest.mark.gpu
def test_run_to_run_identical(gpu):
    masks, scores, _ = fixture()["rect_97x48x70_s1"]
    a = run_nms(gpu, masks, torch.from_numpy(scores), **SITE)
    b = run_nms(gpu, masks, torch.from_numpy(scores), **SITE)
    for x, y in ((a.inter, b.inter), (a.keep, b.keep), (a.selected, b.selected), (a.criteria, b.criteria)):
        assert torch.equal(x, y)
    ranked = masks[a.order.cpu().numpy()]
    assert np.array_equal(a.inter.cpu().numpy(), matmul_table(ranked))


def np_seg_maps(levels, keeps, H, W):
    """mask2segmap (preprocess.py:304-317, the segment map only) per level, then create's offsets (:145-157)."""
    maps, lengths = [], []
    for masks, keep in zip(levels, keeps):
        seg = -np.ones((H, W), dtype=np.int32)
        kept = [] if masks is None else [masks[i] for i in (range(len(masks)) if keep is None else keep)]
        for i, m in enumerate(kept):
            seg[m] = i
        maps.append(seg)
        lengths.append(len(kept))
    for j in range(1, 4):
        maps[j][maps[j] != -1] += sum(lengths[:j])
    return np.stack(maps), lengths


@pytest.mark.gpu
def test_build_seg_maps(gpu):
    from langsplatv2_amd.lang_loss import language_gt_index
    H, W = 37, 53
    M = maker()
    lv0 = M.rect_scene(9, H, W, 11)[0]
    lv0[0] = False
    lv0[0, 5:9, 5:9] = True          # mask 0 lies under masks 1 and 2 together
    lv0[1, 4:10, 4:7] = True
    lv0[2, 4:10, 7:10] = True
    lv2 = M.rect_scene(14, H, W, 12)[0]
    lv3 = M.rect_scene(4, H, W, 13)[0]
    levels = [lv0, np.zeros((0, H, W), dtype=bool), lv2, lv3]
    keep_sets = [[None, None, None, None], [[0, 1, 2, 5, 8], None, [1, 3, 4, 9, 10, 13], [2]]]
    dev_levels = [torch.from_numpy(lv).to(gpu) for lv in levels]
    for keeps in keep_sets:
        want, lengths = np_seg_maps(levels, keeps, H, W)
        assert (want[0][5:9, 5:9] != 0).all()      # fully covered by later masks
        assert (want[1] == -1).all() and lengths[1] == 0
        dev_keeps = [None if k is None else torch.tensor(k, device=gpu) for k in keeps]
        for dtype in (torch.float32, torch.int32):
            got, got_lengths = MN.build_seg_maps(dev_levels, dev_keeps, dtype=dtype)
            assert got.dtype == dtype and tuple(got.shape) == (4, H, W) and got_lengths == lengths
            assert np.array_equal(got.cpu().numpy(), want.astype(got.cpu().numpy().dtype))
        for level in range(4):
            seg = language_gt_index(got, level, gpu)
            assert seg.dtype == torch.int32 and seg.data_ptr() == got[level].data_ptr()   # fed unchanged
            assert np.array_equal(seg.cpu().numpy(), want[level])
    # a level given as None, fewer than four levels, packed input
    got, lengths = MN.build_seg_maps([MN.pack_masks(dev_levels[0]), None, dev_levels[2]], dtype=torch.int32)
    want, _ = np_seg_maps([lv0, None, lv2, None], [None] * 4, H, W)
    assert lengths == [9, 0, 14, 0] and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.gpu
def test_masks_update_filters_in_original_order(gpu):
    names = ["rect_33x40x56_s0", "rect_5x8x9_s1"]
    levels = []
    for name in names:
        masks, scores, _ = fixture()[name]
        levels.append([{"segmentation": masks[i], "predicted_iou": scores[i], "stability_score": np.float64(1.0)}
                       for i in range(len(masks))])
    out = MN.masks_update(*levels, [], device=gpu, **SITE)
    assert isinstance(out, tuple) and len(out) == 3 and out[2] == []
    for name, lvl, got in zip(names, levels, out):
        kept = set(fixture()[name][2].tolist())
        want = [m for i, m in enumerate(lvl) if i in kept]      # the reference's filter
        assert len(got) == len(want) and all(g is w for g, w in zip(got, want))
