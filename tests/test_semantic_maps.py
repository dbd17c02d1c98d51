"""Fused open-vocabulary label maps of the quick path (langsplatv2_amd.semantic,
csrc/quick_semantic.hip) against the reference's OpenCLIPNetwork.get_semantic_map
(eval/openclip_encoder.py:82-94) applied to the float64 decode of the weight map.

tests/golden/ref_semantic.npz holds the reference function's own labels and the
float64 similarities on the fixture of ref_relevancy.npz (make_ref_semantic.py);
`ref_semantic` below is this file's numpy-float64 restatement, pinned to it
(labels exactly, similarities within 1e-12) and used for every other shape.

Bounds (derived, not fitted).  The project holds cosine similarities to
SIM_ATOL = 1e-6 absolute (test_query_relevancy), so two columns can change
places only when their float64 similarities are within 2e-6:
  * for every pixel the float64 similarity of the returned column (for -1: of
    the best negative) is >= the float64 maximum - LABEL_MARGIN = 2e-6, and
  * wherever the float64 top-2 margin is >= 2e-6 the label equals the
    reference's exactly.  No pixel is skipped.
The score p = softmax(scale s)[arg-max] has sum_j |dp/ds_j| = 2 scale p (1 - p)
<= scale / 2, times 1e-6 at scale 10: SCORE_ATOL = 5e-6 absolute, the same
bound as test_query_relevancy.REL_ATOL.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from langsplatv2_amd import _lib, semantic
from test_query_relevancy import DF, K, L, ref_similarity, sparse_map, to_gpu, unit

LABEL_MARGIN = 2e-6
SCORE_ATOL = 5e-6
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_CASES = [(5, 4), (13, 4), (61, 4), (252, 4)]


def _dedup_similarity(wmap, cb, embeds, eps):
    """ref_similarity with identical embedding rows computed once: equal rows
    give equal similarities to the last bit, as they do mathematically (a BLAS
    kernel may sum two equal columns in different orders)."""
    uniq, inverse = np.unique(embeds, axis=0, return_inverse=True)
    return ref_similarity(wmap, cb, uniq, eps)[:, np.asarray(inverse).reshape(-1)]


def ref_semantic(wmap, cb, lab, neg, scale=10.0, eps=1e-10):
    """get_semantic_map in numpy float64: sims (L, H, W, C + N) over
    cat([labels, negatives]), labels (L, H, W) = the first arg-max, -1 where it
    is a negative, scores (L, H, W) = softmax(scale sims) at the arg-max."""
    C = lab.shape[0]
    e = lab if neg is None or neg.shape[0] == 0 else np.concatenate([lab, neg])
    sims = np.ascontiguousarray(np.moveaxis(_dedup_similarity(wmap, cb, e, eps), 1, -1))
    am = sims.argmax(-1)
    labels = np.where(am >= C, -1, am)
    scores = 1.0 / np.exp(scale * (sims - sims.max(-1, keepdims=True))).sum(-1)
    return sims, labels, scores


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN_DIR, "ref_semantic.npz"))
    r = np.load(os.path.join(GOLDEN_DIR, "ref_relevancy.npz"))
    out = dict(wmap=r["weight_map"], cb=r["codebooks"], zero=tuple(int(v) for v in r["zero_pixel"]))
    assert [tuple(c) for c in z["cases"]] == GOLDEN_CASES
    for C, N in GOLDEN_CASES:
        dup = C >= 13
        lab = z["label_table_dup" if dup else "label_table"][:C].astype(np.float32)
        neg = z["neg_embeds_dup" if dup else "neg_embeds"][:N].astype(np.float32)
        sims, labels, scores = ref_semantic(out["wmap"], out["cb"], lab, neg)
        out[(C, N)] = dict(lab=lab, neg=neg, sims=sims, labels=labels, scores=scores,
                           gold_sims=z[f"sims_{C}_{N}"], gold_labels=z[f"labels_{C}_{N}"].astype(np.int64))
    return out


@functools.lru_cache(maxsize=None)
def case(H, W, C, N):
    """Seeded inputs (a fill of 1/16 per channel) and the float64 reference of one shape (read only)."""
    g = np.random.default_rng(H * 1000003 + W * 1009 + C * 7 + N)
    wmap, cb = sparse_map(g, H, W, 1.0 / 16), g.standard_normal((L, K, DF)).astype(np.float32)
    lab, neg = unit(g, C), unit(g, N) if N else None
    sims, labels, scores = ref_semantic(wmap, cb, lab, neg)
    out = dict(wmap=wmap, cb=cb, lab=lab, neg=neg, sims=sims, labels=labels, scores=scores)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def check_labels(got, sims, ref_labels, C, name):
    """The derived label bound of the module docstring, on every pixel."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref_labels.shape and got.dtype == np.int32, name
    n = sims.shape[-1]
    assert got.min() >= -1 and got.max() < C, name
    assert n > C or not (got == -1).any(), f"{name}: -1 without negatives"
    best_neg = C + sims[..., C:].argmax(-1) if n > C else np.zeros_like(got)
    col = np.where(got < 0, best_neg, got)
    took = np.take_along_axis(sims, col[..., None], -1)[..., 0]
    top2 = -np.sort(-sims, axis=-1)[..., :2]
    short = float((top2[..., 0] - took).max())
    clear = (top2[..., 0] - top2[..., -1] >= LABEL_MARGIN) if n > 1 else np.ones(got.shape, bool)
    wrong = int((got[clear] != ref_labels[clear]).sum())
    print(f"{name}: returned column within {short:.3e} of the maximum (bound {LABEL_MARGIN:g}); {int(clear.sum())} of "
          f"{clear.size} pixels with a clear margin, {wrong} of them differ")
    assert short <= LABEL_MARGIN, f"{name}: a returned column is {short:.3e} below the maximum"
    assert wrong == 0, f"{name}: {wrong} labels differ where the float64 margin is >= {LABEL_MARGIN:g}"


def check_scores(got, ref, name):
    got = got.detach().cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all(), name
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{name}: score max abs err {err:.3e} (bound {SCORE_ATOL:g})")
    assert err <= SCORE_ATOL, f"{name}: score max abs err {err:.3e} > {SCORE_ATOL:g}"


def gpu_embeds(c, gpu):
    return to_gpu(c["lab"], gpu), None if c["neg"] is None else to_gpu(c["neg"], gpu)


# ---------------------------------------------------------------- CPU

def test_restatement_matches_reference_golden():
    g = golden()
    zy, zx = g["zero"]
    for C, N in GOLDEN_CASES:
        c = g[(C, N)]
        assert c["labels"].shape == (3, 12, 20)
        np.testing.assert_array_equal(c["labels"], c["gold_labels"])
        mine = c["sims"] if c["gold_sims"].shape[-1] == C + N else -np.sort(-c["sims"], axis=-1)[..., :2]
        assert c["gold_sims"].dtype == np.float64 and np.abs(mine - c["gold_sims"]).max() <= 1e-12
        assert np.all(c["labels"][:, zy, zx] == 0) and np.all(c["scores"][:, zy, zx] == 1.0 / (C + N))
        if C >= 13:
            assert not (c["labels"] == 7).any()          # label 7 is a copy of label 2: the lower column wins
            assert np.array_equal(c["lab"][7], c["lab"][2]) and np.array_equal(c["neg"][1], c["lab"][4])
            assert (c["labels"] == 4).any()              # a negative equal to label 4: the label wins


def test_validation_on_cpu():
    wm, cb, lab, neg = torch.zeros(192, 4, 4), torch.zeros(3, 64, 512), torch.zeros(5, 512), torch.zeros(4, 512)
    with pytest.raises(ValueError):
        semantic.semantic_maps(torch.zeros(4, 4), cb, lab, neg)              # rank
    with pytest.raises(ValueError):
        semantic.semantic_maps(wm, torch.zeros(64, 512), lab, neg)
    with pytest.raises(ValueError):
        semantic.semantic_maps(torch.zeros(100, 4, 4), cb, lab, neg)         # channels != L*K
    with pytest.raises(ValueError):
        semantic.semantic_maps(wm, cb, torch.zeros(5, 256), neg)             # embedding width != Df
    with pytest.raises(ValueError):
        semantic.semantic_maps(wm, cb, lab, torch.zeros(4, 500))
    with pytest.raises(ValueError):
        semantic.semantic_maps(wm, cb, torch.zeros(0, 512), neg)             # no label
    with pytest.raises(ValueError):
        semantic.semantic_maps(wm, cb, torch.zeros(5, 512, dtype=torch.int32), neg)
    with pytest.raises(ValueError):
        semantic.semantic_maps(wm, torch.zeros(3, 32, 512), lab, neg)        # K != 64
    with pytest.raises(ValueError):
        semantic.semantic_maps(wm, cb, lab, neg, scale=-1.0)
    with pytest.raises(ValueError):
        semantic.semantic_maps(wm, cb, lab, neg, scale=float("nan"))
    with pytest.raises(ValueError, match="256"):
        semantic.semantic_maps(wm, cb, torch.zeros(253, 512), neg)           # C + N = 257
    with pytest.raises(ValueError, match="256"):
        semantic.semantic_plan(cb, torch.zeros(257, 512), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        semantic.semantic_maps(wm, cb, lab, neg)
    with pytest.raises(RuntimeError, match="no CPU path"):
        semantic.semantic_plan(cb, lab, neg)
    lb, sc = torch.zeros(3, 4, 4, dtype=torch.int32), torch.zeros(3, 4, 4)
    with pytest.raises(ValueError):
        semantic.merge_levels(lb, torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        semantic.merge_levels(lb.long(), sc)
    with pytest.raises(RuntimeError, match="no CPU path"):
        semantic.merge_levels(lb, sc)
    with pytest.raises(ValueError):
        semantic.label_confusion(torch.zeros(4, dtype=torch.int32), lb[0], 3)
    with pytest.raises(ValueError):
        semantic.label_confusion(sc, lb[0], 3)                               # float labels
    with pytest.raises(ValueError):
        semantic.label_confusion(lb, lb[0], 257)
    with pytest.raises(ValueError):
        semantic.label_confusion(lb, lb[0], 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        semantic.label_confusion(lb, lb[0], 3)
    with pytest.raises(ValueError):
        semantic.semantic_scores(torch.zeros(3, 3))


def test_abi_status_codes_without_device():
    lib = _lib.load()
    f = ctypes.c_float
    nbytes = lib.lsr_quick_semantic_plan_bytes
    assert nbytes(3, 48, 512, 5, 4) == 0
    assert nbytes(3, 64, 500, 5, 4) == 0
    assert nbytes(3, 64, 512, 253, 4) == 0
    assert nbytes(3, 64, 512, 0, 4) == 0
    assert nbytes(3, 64, 512, 252, 4) >= 3 * (16 + 4) * 4096
    assert nbytes(3, 64, 512, 4, 4) == lib.lsr_quick_query_plan_bytes(3, 64, 512, 4, 4)   # the same pieces
    prep = lib.lsr_quick_semantic_prepare
    assert prep(None, None, None, 3, 64, 512, 5, 4, None, None) == 1         # null pointers
    assert prep(None, None, None, 3, 64, 512, 0, 4, None, None) == 1         # no label
    assert prep(None, None, None, 3, 64, 512, 5, -1, None, None) == 1
    assert prep(None, None, None, 3, 48, 512, 5, 4, None, None) == 2         # K != 64
    assert prep(None, None, None, 3, 64, 500, 5, 4, None, None) == 2         # Df % 16 != 0
    assert prep(None, None, None, 3, 64, 512, 253, 4, None, None) == 2       # C + N > 256
    assert prep(None, None, None, 0, 64, 512, 5, 4, None, None) == 0         # L = 0
    run = lib.lsr_quick_semantic_run
    assert run(None, 0, None, 3, 64, 5, 4, 8, 8, f(10), f(1e-10), None, None, None) == 1     # null map
    assert run(None, 2, None, 3, 64, 5, 4, 8, 8, f(10), f(1e-10), None, None, None) == 1     # no such layout
    assert run(None, 0, None, 3, 64, 5, 4, 8, 8, f(-1), f(1e-10), None, None, None) == 1     # negative scale
    assert run(None, 0, None, 3, 64, 5, 4, 8, 8, f(float("nan")), f(1e-10), None, None, None) == 1
    assert run(None, 0, None, 3, 48, 5, 4, 8, 8, f(10), f(1e-10), None, None, None) == 2     # K != 64
    assert run(None, 0, None, 3, 64, 253, 4, 8, 8, f(10), f(1e-10), None, None, None) == 2   # C + N > 256
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                              # (never dereferenced)
    assert run(p + 4, 1, p, 3, 64, 5, 4, 8, 8, f(10), f(1e-10), p, None, None) == 2          # misaligned pixel-major map
    assert run(None, 0, None, 3, 64, 5, 4, 0, 8, f(10), f(1e-10), None, None, None) == 0     # H = 0
    assert run(None, 0, None, 3, 64, 5, 4, 8, 0, f(10), f(1e-10), None, None, None) == 0     # W = 0
    assert run(None, 0, None, 0, 64, 5, 0, 8, 8, f(0), f(1e-10), None, None, None) == 0      # L = 0
    merge = lib.lsr_semantic_merge
    assert merge(None, None, 3, 8, 8, None, None, None) == 1
    assert merge(None, None, -1, 8, 8, None, None, None) == 1
    assert merge(None, None, 256, 8, 8, None, None, None) == 2
    assert merge(None, None, 0, 8, 8, None, None, None) == 0
    assert merge(None, None, 3, 0, 8, None, None, None) == 0
    conf = lib.lsr_semantic_confusion
    assert conf(None, None, 3, 8, 8, 21, None, None) == 1
    assert conf(None, None, 3, 8, 8, 0, None, None) == 1
    assert conf(None, None, 3, 8, 8, 257, None, None) == 2
    assert conf(None, None, 0, 8, 8, 21, None, None) == 0                    # P = 0
    assert conf(None, None, 3, 8, 0, 21, None, None) == 0


def test_semantic_scores_on_a_hand_made_table():
    # rows = gt class, columns = predicted class, last column = predicted -1; class 2 is in neither
    n = np.array([[5, 1, 0, 0, 2],
                  [2, 7, 0, 1, 0],
                  [0, 0, 0, 0, 0],
                  [0, 0, 0, 0, 3]], dtype=np.int64)
    s = semantic.semantic_scores(torch.from_numpy(n))
    row, col, diag = n.sum(1).astype(np.float64), n[:, :4].sum(0).astype(np.float64), np.diag(n[:, :4]).astype(np.float64)
    with np.errstate(invalid="ignore"):
        iou = diag / (row + col - diag)
    assert s.iou.dtype == torch.float64
    np.testing.assert_array_equal(np.isnan(s.iou.numpy()), [False, False, True, False])
    np.testing.assert_allclose(s.iou.numpy()[[0, 1, 3]], iou[[0, 1, 3]], rtol=0, atol=1e-15)
    assert iou[0] == 5 / 10 and iou[1] == 7 / 11 and iou[3] == 0.0
    assert abs(float(s.miou) - (5 / 10 + 7 / 11 + 0.0) / 3) <= 1e-15         # over the classes present in gt
    assert abs(float(s.accuracy) - 12 / 21) <= 1e-15
    both = semantic.semantic_scores(torch.from_numpy(np.stack([n, 2 * n])))  # (P, C, C + 1)
    assert both.iou.shape == (2, 4) and both.miou.shape == (2,)
    np.testing.assert_allclose(both.miou.numpy(), [float(s.miou)] * 2, rtol=0, atol=1e-15)
    empty = semantic.semantic_scores(torch.zeros(2, 3, dtype=torch.int64))
    assert torch.isnan(empty.miou) and torch.isnan(empty.accuracy)


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("C,N", GOLDEN_CASES)
def test_golden(gpu, C, N):
    g = golden()
    c = g[(C, N)]
    zy, zx = g["zero"]
    wm, cb, lab, neg = (to_gpu(a, gpu) for a in (g["wmap"], g["cb"], c["lab"], c["neg"]))
    labels, scores = semantic.semantic_maps(wm, cb, lab, neg, with_scores=True)
    check_labels(labels, c["sims"], c["gold_labels"], C, f"golden C={C} N={N}")
    check_scores(scores, c["scores"], f"golden C={C} N={N}")
    assert torch.equal(labels, semantic.semantic_maps(wm, cb, lab, neg))     # the same bits without scores
    got = labels.cpu().numpy()
    assert np.all(got[:, zy, zx] == 0)
    assert np.all(scores[:, zy, zx].cpu().numpy() == np.float32(1) / np.float32(C + N))
    ref = semantic.get_semantic_map(wm, cb, lab, neg)                        # the drop-in: int64
    assert ref.dtype == torch.int64 and torch.equal(ref, labels.long())
    if C >= 13:
        assert not (got == 7).any()
        # label 4 and its copy among the negatives tie: where label 4 leads the third-best by a clear margin it wins
        top3 = -np.sort(-c["sims"], axis=-1)[..., :3]
        four = (c["sims"].argmax(-1) == 4) & (top3[..., 0] - top3[..., 2] >= LABEL_MARGIN)
        assert four.any() and np.all(got[four] == 4)


SHAPES = [(1, 1), (3, 67), (5, 128), (9, 200)]
COLUMNS = [(1, 0), (1, 1), (12, 4), (13, 4), (60, 4), (61, 4), (252, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
@pytest.mark.parametrize("C,N", COLUMNS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_labels_and_scores_match_float64(gpu, H, W, C, N, hwc):
    c = case(H, W, C, N)
    wm, cb = to_gpu(c["wmap"], gpu, hwc), to_gpu(c["cb"], gpu)
    if hwc and H * W > 1:
        assert wm.stride() == (1, L * K * W, L * K)
    lab, neg = gpu_embeds(c, gpu)
    name = f"{H}x{W} C={C} N={N} {'hwc' if hwc else 'chw'}"
    labels, scores = semantic.semantic_maps(wm, cb, lab, neg, with_scores=True)
    check_labels(labels, c["sims"], c["labels"], C, name)
    check_scores(scores, c["scores"], name)
    only = semantic.semantic_maps(wm, cb, lab, neg)
    assert only.dtype == torch.int32 and torch.equal(only, labels), f"{name}: labels differ without scores"
    if C + N == 1:
        assert torch.all(labels == 0) and torch.all(scores == 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
def test_special_pixels_scale_and_out(gpu, hwc):
    """An all-zero pixel gives label 0 and score 1 / (C + N) exactly; pixels
    scaled down to the subnormal range keep the bound; scale = 0 gives
    1 / (C + N) everywhere; caller-owned outputs are written in place."""
    g = np.random.default_rng(31)
    H, W, C, N = 11, 70, 20, 3
    wmap = sparse_map(g, H, W, 0.2)
    for (y, x), s in {(0, 0): 1e-40, (7, 9): 1e-30, (10, 69): 1e-12, (5, 17): 0.0}.items():
        wmap[:, y, x] = (wmap[:, y, x].astype(np.float64) * s).astype(np.float32)
    cb, lab, neg = g.standard_normal((L, K, DF)).astype(np.float32), unit(g, C), unit(g, N)
    sims, ref_l, ref_s = ref_semantic(wmap, cb, lab, neg)
    t = [to_gpu(a, gpu) for a in (cb, lab, neg)]
    wm = to_gpu(wmap, gpu, hwc)
    out = (torch.full((L, H, W), -7, dtype=torch.int32, device=gpu), torch.full((L, H, W), -7.0, device=gpu))
    labels, scores = semantic.semantic_maps(wm, *t, with_scores=True, out=out)
    assert labels is out[0] and scores is out[1]
    check_labels(labels, sims, ref_l, C, "special pixels")
    check_scores(scores, ref_s, "special pixels")
    assert torch.all(labels[:, 5, 17] == 0) and torch.all(scores[:, 5, 17] == float(np.float32(1) / np.float32(C + N)))
    l0, s0 = semantic.semantic_maps(wm, *t, with_scores=True, scale=0.0)
    assert torch.equal(l0, labels) and torch.all(s0 == float(np.float32(1) / np.float32(C + N)))
    with pytest.raises(ValueError):
        semantic.semantic_maps(wm, *t, out=torch.empty((L, H, W), dtype=torch.int64, device=gpu))


@pytest.mark.gpu
def test_rank_deficient_codebook(gpu):
    """Duplicated codes (a singular Gram matrix), as test_query_relevancy.test_rank_deficient_codebook."""
    g = np.random.default_rng(5)
    wmap, cb, lab, neg = sparse_map(g, 20, 28, 0.2), g.standard_normal((L, K, DF)).astype(np.float32), unit(g, 30), unit(g, 4)
    cb[:, 32:] = cb[:, :32]
    sims, ref_l, ref_s = ref_semantic(wmap, cb, lab, neg)
    labels, scores = semantic.semantic_maps(*(to_gpu(a, gpu) for a in (wmap, cb, lab, neg)), with_scores=True)
    check_labels(labels, sims, ref_l, 30, "rank-32 codebook")
    check_scores(scores, ref_s, "rank-32 codebook")


@pytest.mark.gpu
def test_merge_levels(gpu):
    c = case(9, 200, 61, 4)
    lab, neg = gpu_embeds(c, gpu)
    labels, scores = semantic.semantic_maps(to_gpu(c["wmap"], gpu), to_gpu(c["cb"], gpu), lab, neg, with_scores=True)

    def torch_merge(lb, sc):
        lv = sc.argmax(0)
        return torch.gather(lb, 0, lv[None])[0], lv.to(torch.uint8)

    merged, level = semantic.merge_levels(labels, scores, with_level=True)
    want, want_level = torch_merge(labels, scores)
    assert merged.dtype == torch.int32 and level.dtype == torch.uint8 and merged.shape == (9, 200)
    assert torch.equal(merged, want) and torch.equal(level, want_level)
    assert len(torch.unique(level)) == L                                      # every level wins somewhere
    assert torch.equal(semantic.merge_levels(labels, scores), want)
    # a hand-made tie: equal scores go to the lowest level
    lb = torch.tensor([[[1, 2, 3, 4]], [[5, 6, 7, 8]], [[9, 10, 11, -1]]], dtype=torch.int32, device=gpu)
    sc = torch.tensor([[[0.5, 0.2, 0.1, 0.3]], [[0.5, 0.7, 0.4, 0.3]], [[0.5, 0.7, 0.4, 0.9]]], device=gpu)
    merged, level = semantic.merge_levels(lb, sc, with_level=True)
    assert merged.tolist() == [[1, 6, 7, -1]] and level.tolist() == [[0, 1, 1, 2]]
    want, want_level = torch_merge(lb, sc)
    assert torch.equal(merged, want) and torch.equal(level, want_level)
    one = semantic.merge_levels(lb[:1], sc[:1], with_level=True)
    assert torch.equal(one[0], lb[0]) and not one[1].any()


def numpy_confusion(pred, gt, C):
    counts = np.zeros((pred.shape[0], C, C + 1), dtype=np.int64)
    for p in range(pred.shape[0]):
        ok = (gt >= 0) & (gt < C) & (pred[p] >= -1) & (pred[p] < C)
        np.add.at(counts[p], (gt[ok], np.where(pred[p][ok] < 0, C, pred[p][ok])), 1)
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(7, 13), (64, 200)])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("C", [1, 21, 256])      # 256: the table is too large for LDS, global atomics
def test_label_confusion(gpu, C, P, H, W):
    g = np.random.default_rng(C * 1000 + P * 100 + H)
    pred = g.integers(-1, C, (P, H, W)).astype(np.int32)
    pred[0, 0, :3] = [C, -2, 1 << 30]                                         # outside [-1, C): skipped
    gt = g.integers(0, C, (H, W)).astype(np.int64)
    ignore = g.random((H, W))
    gt[ignore < 0.1] = 255 if C < 256 else 256                                # ignore labels
    gt[ignore > 0.9] = -1
    pred[:, -1, -3:], gt[-1, -3:] = -1, [0, C - 1, C // 2]                    # -1 predictions on annotated pixels
    want = numpy_confusion(pred, gt, C)
    tp, tg = torch.from_numpy(pred).to(gpu), torch.from_numpy(gt).to(gpu)
    got = semantic.label_confusion(tp, tg, C)
    assert got.dtype == torch.int64 and got.shape == (P, C, C + 1)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert 0 < int(got.sum()) < P * H * W and int(got[:, :, C].sum()) > 0     # pixels were skipped, -1 was counted
    assert torch.equal(got, semantic.label_confusion(tp, tg, C))              # two calls, the same table
    single = semantic.label_confusion(tp[0], tg, C)                           # (H, W) pred
    assert single.shape == (C, C + 1) and torch.equal(single, got[0])
    assert torch.equal(semantic.label_confusion(tp.long(), tg.int(), C), got)  # other integer dtypes
    if H % 2 == 0 and W % 2 == 0:
        # a half-size annotation: cv2.INTER_NEAREST to twice the size takes source index x // 2
        small = np.ascontiguousarray(gt[::2, ::2])
        up = small[np.arange(H) // 2][:, np.arange(W) // 2]
        got2 = semantic.label_confusion(tp, torch.from_numpy(small).to(gpu), C)
        np.testing.assert_array_equal(got2.cpu().numpy(), numpy_confusion(pred, up, C))


@pytest.mark.gpu
def test_plan_cache(gpu):
    g = np.random.default_rng(6)
    wmap, cbn, labn, negn = sparse_map(g, 16, 24, 0.2), g.standard_normal((L, K, DF)).astype(np.float32), unit(g, 20), unit(g, 4)
    wm, cb, lab, neg = (to_gpu(a, gpu) for a in (wmap, cbn, labn, negn))
    p0 = semantic.semantic_plan(cb, lab, neg)
    assert p0.buf.numel() == _lib.load().lsr_quick_semantic_plan_bytes(L, K, DF, 20, 4)
    a = semantic.semantic_maps(wm, cb, lab, neg)
    assert semantic.semantic_plan(cb, lab, neg) is p0                        # the same label set across frames
    assert torch.equal(a, semantic.semantic_maps(wm, cb, lab, neg))
    cb.mul_(-0.5)                                                             # in place: the version counter moves
    assert semantic.semantic_plan(cb, lab, neg) is not p0
    sims, ref_l, _ = ref_semantic(wmap, cb.cpu().numpy(), labn, negn)
    check_labels(semantic.semantic_maps(wm, cb, lab, neg), sims, ref_l, 20, "after codebook update")
    p1 = semantic.semantic_plan(cb, lab, neg)
    lab2n = unit(g, 20)
    lab2 = to_gpu(lab2n, gpu)                                                 # a new label set
    assert semantic.semantic_plan(cb, lab2, neg) is not p1
    sims, ref_l, _ = ref_semantic(wmap, cb.cpu().numpy(), lab2n, negn)
    check_labels(semantic.semantic_maps(wm, cb, lab2, neg), sims, ref_l, 20, "new label set")
    assert semantic.semantic_plan(cb, lab2, None) is not semantic.semantic_plan(cb, lab2, neg)
    # fp16 embeddings (the reference's dtype): cast to fp32 and used as given
    lh, nh = lab2.half(), neg.half()
    sims, ref_l, _ = ref_semantic(wmap, cb.cpu().numpy(), lh.float().cpu().numpy(), nh.float().cpu().numpy())
    check_labels(semantic.semantic_maps(wm, cb, lh, nh), sims, ref_l, 20, "fp16 embeddings")
    assert semantic.semantic_plan(cb, lh, nh) is semantic.semantic_plan(cb, lh, nh)


@pytest.mark.gpu
@pytest.mark.parametrize("with_scores", [False, True], ids=["labels", "scores"])
def test_semantic_stream(gpu, with_scores):
    """QuickSemanticStream over 3 pushed maps equals the direct calls bit for
    bit, from the default stream and from inside a non-default caller stream."""
    g = np.random.default_rng(9)
    maps = [to_gpu(sparse_map(g, 33, 52), gpu, hwc=bool(i & 1)) for i in range(3)]
    cb = to_gpu(g.standard_normal((L, K, DF)).astype(np.float32), gpu)
    lab, neg = to_gpu(unit(g, 40), gpu), to_gpu(unit(g, 4), gpu)
    ref = [semantic.semantic_maps(m, cb, lab, neg, with_scores=with_scores) for m in maps]
    torch.cuda.synchronize()

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b)) if with_scores else torch.equal(a, b)

    def run():
        ss = semantic.QuickSemanticStream(cb, lab, neg, with_scores=with_scores)
        got = [ss.push(lambda m=m: m) for m in maps]
        assert got[0] is None
        got = got[1:] + [ss.flush()]
        assert ss.flush() is None
        return got

    got = run()
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(got, ref))
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        got = run()
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(got, ref))


@pytest.mark.gpu
def test_render_then_labels_then_confusion_end_to_end(gpu, oracle_lib):
    """Quick render through the drop-in rasterizer at its default (pixel-major)
    layout -> semantic_maps -> merge_levels -> label_confusion -> semantic_scores,
    against the restatement on the oracle's weight map."""
    from harness import make_case, oracle_problem
    from test_quick_stream import _renderer
    case_ = make_case(N=3000, W=96, H=80, seed=21, sh_degree=None, quick_k=4)
    ref_f = oracle_lib.forward(oracle_problem(case_))
    wm = _renderer(case_, gpu, None)()
    assert wm.stride() == (1, 192 * 96, 192)                                  # the default layout is pixel-major
    np.testing.assert_array_equal(wm.cpu().numpy(), ref_f["lang"])
    g = np.random.default_rng(3)
    C = 21
    cb, lab, neg = g.standard_normal((L, K, DF)).astype(np.float32), unit(g, C), unit(g, 4)
    sims, ref_l, ref_s = ref_semantic(ref_f["lang"], cb, lab, neg)
    labels, scores = semantic.semantic_maps(wm, *(to_gpu(a, gpu) for a in (cb, lab, neg)), with_scores=True)
    check_labels(labels, sims, ref_l, C, "render + labels")
    check_scores(scores, ref_s, "render + labels")
    merged = semantic.merge_levels(labels, scores)
    gt = ref_l[0].copy()                                                      # level 0 of the reference as annotation
    gt[:8] = 255
    planes = torch.cat([labels, merged[None]])
    counts = semantic.label_confusion(planes, torch.from_numpy(gt).to(gpu), C)
    np.testing.assert_array_equal(counts.cpu().numpy(), numpy_confusion(planes.cpu().numpy(), gt, C))
    s = semantic.semantic_scores(counts)
    # level 0 against its own reference: every counted pixel outside the label margin is on the diagonal
    top = np.sort(sims[0], axis=-1)
    unclear = int((top[..., -1] - top[..., -2] < LABEL_MARGIN)[8:].sum())
    counted, correct = int(counts[0].sum()), int(torch.diagonal(counts[0, :, :C]).sum())
    assert counted == int(((gt >= 0) & (gt < C)).sum()) > 0 and correct >= counted - unclear
    assert float(s.accuracy[0]) == correct / counted and 0.0 <= float(s.miou[3]) <= 1.0
