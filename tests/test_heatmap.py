"""Fused query heatmap frames of the viewer path (langsplatv2_amd.heatmap,
csrc/quick_heat.hip) against numpy restatements of the reference's two
interactive consumers, which import cv2 and zmq at module level and cannot be
imported here:

  backend_renderer.py:204-233  sum of the normalised level features,
      renormalised, cosine with the prompt; min / max, two gates, the "upper
      half of the range" normalisation, colour table, 50/50 blend, uint8
  demo_prompt.py:122-137       get_max_across_quick(...).mean(0); min / max,
      one gate, normalise, ** 4, colour table

Tolerances (derived, not fitted).  Summed cosine, HEAT_ATOL = 1e-5 absolute:
the project holds each per-level cosine to 1e-6 (SIM_ATOL), so the numerator
s . e is off by at most L 1e-6 = 3e-6; |s|^2 is a sum of L^2 such cosines, so
delta |s| <= 9e-6 / (2 |s|); with |s . e| <= |s| and |s| >= 1 the quotient is
off by at most 3e-6 + 4.5e-6 < 1e-5.  |s| >= 1 on every non-zero pixel is a
condition of that bound and is asserted on the float64 reference (the seeded
maps give min |s| = 1.34 .. 1.78).  Mean relevancy: a mean of values each held
to REL_ATOL = 5e-6.  The colour stage is fp32 with every operation rounded on
its own, so the numpy-float32 restatement below must give the kernel's bytes.

Measured on the MI355X over this file's cases: summed cosine <= 8.5e-8, mean
relevancy <= 1.2e-7 ("Query heatmap frames").
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from langsplatv2_amd import _lib, heatmap, query
from test_query_relevancy import (DF, K, L, QUERIES, REL_ATOL, SHAPES, case, check, ref_relevancy, sparse_map, to_gpu,
                                  unit)
from test_quick_decode import ref_decode

HEAT_ATOL = 1e-5
SUMMED_Q = [1, 13, 3, 20]       # the server's single prompt; the query counts of QUERIES; two 16-column blocks (the
                                # stacked factor then no longer fits the LDS beside the projections at L = 3)
F32 = np.float32


# ---------------------------------------------------------------- restatements

def ref_summed(wmap, cb, embeds, eps=1e-10):
    """backend_renderer.py:204-210 in float64 -> (Q, H, W) and |s| (H, W)."""
    F = ref_decode(wmap, cb, True, eps)                                   # (L, Df, H, W)
    s = F.sum(axis=0)
    n = np.linalg.norm(s, axis=0)
    return np.einsum("dhw,qd->qhw", s / (n + eps), embeds.astype(np.float64)), n


def ref_mean_relevancy(wmap, cb, pos, neg, scale=10.0, eps=1e-10):
    return ref_relevancy(wmap, cb, pos, neg, scale, eps).mean(axis=0)


def np_heat_frames(maps, lut, rgb=None, curve="upper_half", threshold=0.22, min_range=0.02, alpha=0.5):
    """The colour stage in numpy float32, operation for operation as
    include/lsr.h states it (lsr_heat_frame)."""
    maps = np.asarray(maps, dtype=F32)
    P, H, W = maps.shape
    out = np.empty((P, H, W, 3), dtype=np.uint8)
    for p in range(P):
        x = maps[p]
        mn, mx = x.min(), x.max()
        if mx < F32(threshold) or (mx - mn) < F32(min_range):
            v = np.zeros_like(x)
        elif curve == "upper_half":
            t = (x - mn) / ((mx - mn) + F32(1e-9))
            v = np.minimum(np.maximum(t * F32(2) - F32(1), F32(0)), F32(1))
        else:
            t = (x - mn) / ((mx - mn) + F32(1e-8))
            v = (t * t) * (t * t)
        assert v.dtype == F32
        idx = np.clip((v * F32(255)).astype(np.int32), 0, 255)
        heat = lut[idx]                                                   # (H, W, 3) uint8
        if rgb is None:
            out[p] = heat
        else:
            c = rgb.transpose(1, 2, 0) * (F32(1) - F32(alpha)) + (heat.astype(F32) / F32(255)) * F32(alpha)
            assert c.dtype == F32
            out[p] = (np.minimum(np.maximum(c, F32(0)), F32(1)) * F32(255)).astype(np.uint8)
    return out


def ref64_heat_index(maps, curve, threshold=0.22, min_range=0.02):
    """The reference's formulas in float64 up to the table index
    (backend_renderer.py:38-55, 215-230; demo_prompt.py:126-137)."""
    out = np.empty(maps.shape, dtype=np.int64)
    for p, x in enumerate(maps.astype(np.float64)):
        mn, mx = x.min(), x.max()
        if mx < threshold or mx - mn < min_range:
            v = np.zeros_like(x)
        elif curve == "upper_half":
            v = np.clip((x - mn) / (mx - mn + 1e-9) * 2 - 1, 0, 1)
        else:
            v = ((x - mn) / (mx - mn + 1e-8)) ** 4
        out[p] = np.floor(v * 255)
    return out


def identity_lut():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


@functools.lru_cache(maxsize=None)
def summed_case(H, W, Q):
    """Seeded inputs (the map and codebooks of test_query_relevancy.case) and
    the float64 reference of one shape, shared by the tests (read only)."""
    c = case(H, W, 1, 4)
    e = unit(np.random.default_rng(H * 1000 + W * 10 + Q), Q)
    ref, n = ref_summed(c["wmap"], c["cb"], e)
    nz = np.abs(c["wmap"]).reshape(L, K, H, W).max(axis=1).max(axis=0) > 0
    out = dict(wmap=c["wmap"], cb=c["cb"], e=e, ref=ref, norm=n, nonzero=nz)
    for v in out.values():
        v.setflags(write=False)
    return out


def seeded_planes(g, H, W):
    """Four planes: a relevancy-like one, a cosine-like one with negative
    values, one whose maximum is below 0.22 and one with range below 0.02."""
    a = 1.0 / (1.0 + np.exp(-3.0 * g.standard_normal((H, W))))
    b = 0.45 * np.tanh(g.standard_normal((H, W)))
    c = 0.2 * g.random((H, W))
    d = 0.5 + 0.015 * g.random((H, W))
    return np.stack([a, b, c, d]).astype(F32)


def mixed_prompt(g, cb, noise=0.5):
    """A unit prompt along a mix of codebook rows plus noise: unlike a random
    unit vector (cosines near +-0.2 at most, which only exercises the gate) it
    is well inside the span the decoded features live in."""
    w = g.random(cb.shape[:2])
    e = np.einsum("lk,lkd->d", w, cb.astype(np.float64))
    e = e / np.linalg.norm(e) + noise * g.standard_normal(cb.shape[2]) / np.sqrt(cb.shape[2])
    return (e / np.linalg.norm(e)).astype(F32)[None]


# ---------------------------------------------------------------- CPU

def test_validation_on_cpu():
    wm, cb, pos, neg = torch.zeros(192, 4, 4), torch.zeros(3, 64, 512), torch.zeros(2, 512), torch.zeros(4, 512)
    for f, extra in ((heatmap.summed_similarity_maps, ()), (heatmap.mean_relevancy_maps, (neg,))):
        with pytest.raises(ValueError):
            f(torch.zeros(4, 4), cb, pos, *extra)                          # rank
        with pytest.raises(ValueError):
            f(wm, torch.zeros(64, 512), pos, *extra)
        with pytest.raises(ValueError):
            f(torch.zeros(100, 4, 4), cb, pos, *extra)                     # channels != L*K
        with pytest.raises(ValueError):
            f(wm, cb, torch.zeros(2, 256), *extra)                         # embedding width != Df
        with pytest.raises(ValueError):
            f(torch.zeros(256, 4, 4), torch.zeros(4, 64, 512), pos, *extra)   # four levels
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(wm, cb, pos, *extra)
    with pytest.raises(ValueError):
        heatmap.mean_relevancy_maps(wm, cb, pos, torch.zeros(4, 500))
    with pytest.raises(ValueError):
        heatmap.mean_relevancy_maps(wm, cb, pos, neg, scale=-1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        heatmap.heat_plan(cb, pos, neg)
    maps, lut, rgb = torch.zeros(2, 4, 4), torch.zeros(256, 3, dtype=torch.uint8), torch.zeros(3, 4, 4)
    with pytest.raises(ValueError):
        heatmap.heat_frames(torch.zeros(4, 4), lut)                        # rank
    with pytest.raises(ValueError):
        heatmap.heat_frames(maps.double(), lut)
    with pytest.raises(ValueError):
        heatmap.heat_frames(maps, torch.zeros(256, 3))                     # table dtype
    with pytest.raises(ValueError):
        heatmap.heat_frames(maps, lut[:255])
    with pytest.raises(ValueError):
        heatmap.heat_frames(maps, lut, rgb=torch.zeros(3, 4, 5))
    with pytest.raises(ValueError):
        heatmap.heat_frames(maps, lut, curve="sqrt")
    with pytest.raises(ValueError):
        heatmap.heat_frames(maps, lut, alpha=1.5)
    with pytest.raises(ValueError):
        heatmap.heat_frames(maps, lut, alpha=float("nan"))
    with pytest.raises(ValueError):
        heatmap.heat_frames(torch.zeros(0, 4, 4), lut)
    with pytest.raises(RuntimeError, match="no CPU path"):
        heatmap.heat_frames(maps, lut)
    with pytest.raises(RuntimeError, match="no CPU path"):
        heatmap.heat_frames(maps, lut, rgb=rgb, curve="power4")


def test_abi_status_codes_without_device():
    lib = _lib.load()
    f = ctypes.c_float
    assert lib.lsr_quick_heat_plan_bytes(3, 48, 512, 3, 4) == 0           # K != 64
    assert lib.lsr_quick_heat_plan_bytes(3, 64, 500, 3, 4) == 0           # Df no multiple of 16
    assert lib.lsr_quick_heat_plan_bytes(4, 64, 512, 3, 4) == 0           # four levels
    assert lib.lsr_quick_heat_plan_bytes(3, 64, 512, 61, 4) == 0          # 61 + 4 columns
    assert lib.lsr_quick_heat_plan_bytes(3, 64, 512, 1, 0) >= 3 * (1 + 4 + 8) * 4096
    assert lib.lsr_quick_query_plan_bytes(3, 64, 512, 4, 4) == 172544     # the query plan did not grow
    run = lib.lsr_quick_heat_run
    assert run(None, 0, None, 3, 64, 1, 0, 8, 8, 0, f(0), f(1e-10), None, None) == 1         # null map
    assert run(None, 2, None, 3, 64, 1, 0, 8, 8, 0, f(0), f(1e-10), None, None) == 1         # no such layout
    assert run(None, 0, None, 3, 64, 1, 0, 8, 8, 2, f(0), f(1e-10), None, None) == 1         # no such mode
    assert run(None, 0, None, 3, 64, 1, 4, 8, 8, 1, f(-1), f(1e-10), None, None) == 1        # negative scale
    assert run(None, 0, None, 3, 64, 1, 4, 8, 8, 1, f(float("nan")), f(1e-10), None, None) == 1
    assert run(None, 0, None, 3, 64, 61, 4, 8, 8, 0, f(0), f(1e-10), None, None) == 2        # n_pos + n_neg > 64
    assert run(None, 0, None, 3, 48, 1, 0, 8, 8, 0, f(0), f(1e-10), None, None) == 2         # K != 64
    assert run(None, 0, None, 4, 64, 1, 0, 8, 8, 0, f(0), f(1e-10), None, None) == 2         # four levels
    assert run(None, 0, None, 3, 64, 3, 0, 8, 8, 1, f(10), f(1e-10), None, None) == 2        # mean relevancy, no negatives
    assert run(None, 0, None, 3, 64, 1, 0, 0, 8, 0, f(0), f(1e-10), None, None) == 0         # H = 0
    assert run(None, 0, None, 0, 64, 1, 4, 8, 8, 1, f(10), f(1e-10), None, None) == 0        # L = 0
    prep = lib.lsr_quick_heat_prepare
    assert prep(None, None, None, 3, 64, 512, 3, 4, None, None) == 1
    assert prep(None, None, None, 3, 64, 512, 0, 4, None, None) == 1
    assert prep(None, None, None, 3, 64, 512, 61, 4, None, None) == 2
    assert prep(None, None, None, 4, 64, 512, 3, 4, None, None) == 2
    assert prep(None, None, None, 0, 64, 512, 3, 4, None, None) == 0
    frame = lib.lsr_heat_frame
    assert frame(None, None, None, None, 1, 8, 8, 0, f(0.22), f(0.02), f(0.5), None, None) == 1      # null maps
    assert frame(None, None, None, None, 1, 8, 8, 2, f(0.22), f(0.02), f(0.5), None, None) == 1      # no such curve
    assert frame(None, None, None, None, 1, 8, 8, 0, f(0.22), f(0.02), f(-0.5), None, None) == 1
    assert frame(None, None, None, None, 1, 8, 8, 0, f(0.22), f(0.02), f(1.5), None, None) == 1
    assert frame(None, None, None, None, 1, 8, 8, 1, f(0.22), f(0.02), f(float("nan")), None, None) == 1
    assert frame(None, None, None, None, 70000, 8, 8, 0, f(0.22), f(0.02), f(0.5), None, None) == 2  # planes
    assert frame(None, None, None, None, 0, 8, 8, 0, f(0.22), f(0.02), f(0.5), None, None) == 0
    assert frame(None, None, None, None, 1, 8, 0, 1, f(0.22), f(0.0), f(1.0), None, None) == 0


def test_jet_lut():
    lut = heatmap.jet_lut().numpy().astype(np.int64)
    assert lut.shape == (256, 3) and heatmap.jet_lut().dtype == torch.uint8
    assert tuple(lut[0]) == (0, 0, 128) and tuple(lut[255]) == (128, 0, 0)
    r, g, b = lut.T
    # the piecewise-linear shape: each channel rises, holds 255, falls, and is 0 elsewhere
    for ch, up, top, down in ((r, (96, 159), (160, 223), (224, 255)), (g, (32, 95), (96, 159), (160, 223)),
                              (b, (0, 31), (32, 95), (96, 159))):
        assert np.all(np.diff(ch[up[0]:up[1] + 1]) > 0)
        assert np.all(ch[top[0]:top[1] + 1] >= 251) and ch[top[0]:top[1] + 1].max() == 255
        assert np.all(np.diff(ch[down[0]:down[1] + 1]) < 0)
    assert np.all(r[:95] == 0) and np.all(g[:31] == 0) and np.all(g[224:] == 0) and np.all(b[160:] == 0)
    x = np.arange(256) / 255.0
    want = np.floor(np.clip(1.5 - np.abs(4 * x[:, None] - np.array([3.0, 2.0, 1.0])), 0, 1) * 255 + 0.5)
    np.testing.assert_array_equal(lut, want.astype(np.int64))


@pytest.mark.parametrize("curve", ["upper_half", "power4"])
def test_float32_restatement_within_one_index_of_float64(curve):
    g = np.random.default_rng(41)
    maps = seeded_planes(g, 37, 45)
    got = np_heat_frames(maps, identity_lut(), None, curve, 0.22, 0.02 if curve == "upper_half" else 0.0)
    assert np.all(got[..., 0] == got[..., 1]) and np.all(got[..., 0] == got[..., 2])
    ref = ref64_heat_index(maps, curve, 0.22, 0.02 if curve == "upper_half" else 0.0)
    d = np.abs(got[..., 0].astype(np.int64) - ref)
    print(f"{curve}: {int((d > 0).sum())} of {d.size} indices differ, max {int(d.max())}")
    assert d.max() <= 1
    assert np.all(got[2] == 0)                                            # maximum below the threshold
    assert np.all(got[3] == 0) == (curve == "upper_half")                 # the range gate is the server's only
    assert got[0].max() == 255 or got[0].max() == 254


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
@pytest.mark.parametrize("Q", SUMMED_Q)
@pytest.mark.parametrize("H,W", SHAPES)
def test_summed_cosine_matches_float64(gpu, H, W, Q, hwc):
    c = summed_case(H, W, Q)
    assert c["norm"][c["nonzero"]].min() >= 1.0                           # the bound's condition
    wm = to_gpu(c["wmap"], gpu, hwc)
    if hwc and H * W > 1:
        assert wm.stride() == (1, L * K * W, L * K)
    got = heatmap.summed_similarity_maps(wm, to_gpu(c["cb"], gpu), to_gpu(c["e"], gpu))
    check(got, c["ref"], HEAT_ATOL, f"summed cosine {H}x{W} Q={Q} {'hwc' if hwc else 'chw'}")


@pytest.mark.gpu
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
@pytest.mark.parametrize("Q,N", QUERIES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_mean_relevancy_matches_float64(gpu, H, W, Q, N, hwc):
    c = case(H, W, Q, N)
    got = heatmap.mean_relevancy_maps(to_gpu(c["wmap"], gpu, hwc), to_gpu(c["cb"], gpu), to_gpu(c["pos"], gpu),
                                      to_gpu(c["neg"], gpu))
    check(got, c["rel"].mean(axis=0), REL_ATOL, f"mean relevancy {H}x{W} Q={Q} N={N} {'hwc' if hwc else 'chw'}")


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2])
def test_fewer_levels(gpu, levels):
    """L = 1 (|s| = |f_0|: the level's own cosine) and L = 2."""
    g = np.random.default_rng(20 + levels)
    H, W = 19, 37
    wmap = sparse_map(g, H, W, 0.2)[:levels * K]
    cb, pos, neg = g.standard_normal((levels, K, DF)).astype(F32), unit(g, 5), unit(g, 4)
    t = [to_gpu(a, gpu) for a in (wmap, cb, pos, neg)]
    ref, n = ref_summed(wmap, cb, pos)
    assert n.min() >= (1.0 if levels > 1 else 1.0 - 1e-9)
    check(heatmap.summed_similarity_maps(*t[:3]), ref, HEAT_ATOL, f"summed cosine L={levels}")
    check(heatmap.mean_relevancy_maps(*t), ref_mean_relevancy(wmap, cb, pos, neg), REL_ATOL,
          f"mean relevancy L={levels}")


@pytest.mark.gpu
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
def test_special_pixels(gpu, hwc):
    """An all-zero pixel gives exactly 0 / 0.5; a pixel with one level zero
    and pixels scaled by 1e-12 (|F| comparable to eps), 1e-20 and 1e-40
    (subnormal) stay finite and within tolerance; every other pixel keeps the
    bits it has without them."""
    g = np.random.default_rng(12)
    H, W = 24, 40
    base = sparse_map(g, H, W, 0.2)
    wmap = base.copy()
    special = {(0, 0): 1e-40, (11, 20): 1e-20, (23, 39): 1e-12, (5, 17): 0.0}
    for (y, x), s in special.items():
        wmap[:, y, x] = (wmap[:, y, x].astype(np.float64) * s).astype(F32)
    wmap[K:2 * K, 9, 3] = 0.0                                             # level 1 alone is empty here
    wmap[:K, 16, 33] = 0.0
    wmap[2 * K:, 16, 33] = 0.0                                            # only level 1 is left here
    special[(9, 3)] = special[(16, 33)] = None
    cb, pos, neg = g.standard_normal((L, K, DF)).astype(F32), unit(g, 3), unit(g, 4)
    t = [to_gpu(a, gpu) for a in (cb, pos, neg)]
    ref, n = ref_summed(wmap, cb, pos)
    keep = np.ones((H, W), dtype=bool)
    for (y, x) in special:
        keep[y, x] = False
    assert n[keep].min() >= 1.0 and n[9, 3] >= 1.0 and abs(n[16, 33] - 1.0) < 1e-9
    got = heatmap.summed_similarity_maps(to_gpu(wmap, gpu, hwc), t[0], t[1])
    rel = heatmap.mean_relevancy_maps(to_gpu(wmap, gpu, hwc), *t)
    check(got, ref, HEAT_ATOL, "special pixels summed cosine")
    check(rel, ref_mean_relevancy(wmap, cb, pos, neg), REL_ATOL, "special pixels mean relevancy")
    assert torch.all(got[:, 5, 17] == 0.0) and torch.all(rel[:, 5, 17] == 0.5)
    keep_t = torch.tensor(keep, device=gpu)
    got0 = heatmap.summed_similarity_maps(to_gpu(base, gpu, hwc), t[0], t[1])
    rel0 = heatmap.mean_relevancy_maps(to_gpu(base, gpu, hwc), *t)
    assert torch.equal(got[:, keep_t], got0[:, keep_t]) and torch.equal(rel[:, keep_t], rel0[:, keep_t])


@pytest.mark.gpu
def test_identical_levels(gpu):
    """cb[1] = cb[2] = cb[0] and the same weights per level: the stacked Gram
    matrix is singular (rank 64), |s| = 3 and the summed cosine is the level's."""
    g = np.random.default_rng(31)
    H, W = 21, 36
    one = sparse_map(g, H, W, 0.2)[:K]
    wmap = np.concatenate([one, one, one])
    cb1 = g.standard_normal((1, K, DF)).astype(F32)
    cb, e = np.concatenate([cb1, cb1, cb1]), unit(g, 3)
    ref, n = ref_summed(wmap, cb, e)
    assert np.abs(n - 3.0).max() < 1e-8
    t = [to_gpu(a, gpu) for a in (wmap, cb, e)]
    got = heatmap.summed_similarity_maps(*t)
    check(got, ref, HEAT_ATOL, "identical levels vs float64")
    sim = query.similarity_maps(*t)[0]
    err = float((got - sim).abs().max())
    print(f"identical levels vs similarity_maps: {err:.3e} (bound 2e-6)")
    assert err <= 2e-6


@pytest.mark.gpu
def test_cancelling_levels(gpu):
    """cb[1] = -cb[0] with equal weights plus a random third level: f_0 + f_1
    = 0, |s| = |f_2| = 1 and the result is level 2's cosine.  A |s|^2 formed as
    a difference of O(1) terms loses this case; the sum of squares does not."""
    g = np.random.default_rng(32)
    H, W = 21, 36
    wmap = sparse_map(g, H, W, 0.2)
    wmap[K:2 * K] = wmap[:K]
    cb, e = g.standard_normal((L, K, DF)).astype(F32), unit(g, 3)
    cb[1] = -cb[0]
    ref, n = ref_summed(wmap, cb, e)
    assert np.abs(n - 1.0).max() < 1e-9                                   # |s| = 1: the bound's condition, at its edge
    t = [to_gpu(a, gpu) for a in (wmap, cb, e)]
    got = heatmap.summed_similarity_maps(*t)
    check(got, ref, HEAT_ATOL, "cancelling levels vs float64")
    lvl2 = np.einsum("dhw,qd->qhw", ref_decode(wmap, cb)[2], e.astype(np.float64))
    check(got, lvl2, HEAT_ATOL, "cancelling levels vs level 2's cosine")


@pytest.mark.gpu
@pytest.mark.parametrize("with_rgb", [False, True], ids=["heat", "blend"])
@pytest.mark.parametrize("curve", ["upper_half", "power4"])
@pytest.mark.parametrize("H,W", [(37, 45), (64, 128), (1, 1)])
def test_colour_stage_bytes(gpu, H, W, curve, with_rgb):
    """heat_frames equals the numpy-float32 restatement byte for byte: a live
    plane of each kind, one plane per gate (maximum below the threshold, range
    below min_range, a constant plane), RGB values below 0 and above 1, and
    the same bytes from a second run."""
    g = np.random.default_rng(H * 7 + W)
    maps = np.concatenate([seeded_planes(g, H, W), np.full((1, H, W), 0.6, dtype=F32)])
    rgb = (g.random((3, H, W)) * 1.4 - 0.2).astype(F32) if with_rgb else None
    lut = heatmap.jet_lut().numpy()
    kw = dict(curve=curve, threshold=0.22, min_range=0.02 if curve == "upper_half" else 0.0, alpha=0.5)
    want = np_heat_frames(maps, lut, rgb, **kw)
    m, lt = to_gpu(maps, gpu), to_gpu(lut, gpu)
    r = None if rgb is None else to_gpu(rgb, gpu)
    got = heatmap.heat_frames(m, lt, rgb=r, **kw)
    assert got.shape == (5, H, W, 3) and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, heatmap.heat_frames(m, lt, rgb=r, **kw))
    if rgb is None and H * W > 1:
        assert np.all(want[2] == lut[0]) and np.all(want[4] == lut[0])    # gated planes take the table's first entry
        assert len(np.unique(want[0].reshape(-1, 3), axis=0)) > 16         # and a live plane is live
    # another alpha and an identity table
    if with_rgb:
        kw2 = dict(kw, alpha=0.25)
        got2 = heatmap.heat_frames(m, to_gpu(identity_lut(), gpu), rgb=r, **kw2)
        np.testing.assert_array_equal(got2.cpu().numpy(), np_heat_frames(maps, identity_lut(), rgb, **kw2))


@pytest.mark.gpu
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
def test_end_to_end_frames(gpu, hwc):
    """heat_frames(summed_similarity_maps(...), rgb=...) and the demo's
    heat_frames(mean_relevancy_maps(...), curve="power4") equal the restatement
    applied to the kernel's own map byte for byte (the map itself is held to
    float64 above), on a prompt whose float64 map passes both gates."""
    H, W = 37, 45
    c = case(H, W, 1, 4)
    g = np.random.default_rng(77)
    e = mixed_prompt(g, c["cb"])
    ref, _ = ref_summed(c["wmap"], c["cb"], e)
    print(f"float64 summed cosine: min {ref.min():.4f} max {ref.max():.4f}")
    assert ref.max() >= 0.22 and ref.max() - ref.min() >= 0.02
    rgb = (g.random((3, H, W)) * 1.2 - 0.1).astype(F32)
    wm, cb, et, rt = to_gpu(c["wmap"], gpu, hwc), to_gpu(c["cb"], gpu), to_gpu(e, gpu), to_gpu(rgb, gpu)
    lut = heatmap.jet_lut(gpu)
    maps = heatmap.summed_similarity_maps(wm, cb, et)
    check(maps, ref, HEAT_ATOL, "end to end summed cosine")
    got = heatmap.heat_frames(maps, lut, rgb=rt)
    want = np_heat_frames(maps.cpu().numpy(), lut.cpu().numpy(), rgb)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 64
    # the demo: mean relevancy, 0.22 gate only, 4th power, no blend
    neg = to_gpu(c["neg"], gpu)
    rel = heatmap.mean_relevancy_maps(wm, cb, et, neg)
    relref = ref_mean_relevancy(c["wmap"], c["cb"], e, c["neg"])
    assert relref.max() >= 0.22
    check(rel, relref, REL_ATOL, "end to end mean relevancy")
    got = heatmap.heat_frames(rel, lut, curve="power4", min_range=0.0)
    np.testing.assert_array_equal(got.cpu().numpy(),
                                  np_heat_frames(rel.cpu().numpy(), lut.cpu().numpy(), None, "power4", 0.22, 0.0))


@pytest.mark.gpu
def test_render_then_frame_end_to_end(gpu, oracle_lib):
    """Quick render through the drop-in rasterizer at its default (pixel-major)
    layout, then the server's frame: map vs float64 on the oracle's weight
    map, frame vs the restatement on the kernel's map and the rasterizer's image."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from harness import make_case, oracle_problem, settings_for
    case_ = make_case(N=3000, W=96, H=80, seed=21, sh_degree=None, quick_k=4)
    ref_f = oracle_lib.forward(oracle_problem(case_))
    t = {k: v.to(gpu) for k, v in case_["g"].items() if isinstance(v, torch.Tensor)}
    r = GaussianRasterizer(raster_settings=settings_for(case_, gpu, None))
    with torch.no_grad():
        res = r(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"],
                language_feature_weights_quick=t["language_feature_weights_quick"],
                language_feature_indices=t["language_feature_indices"],
                **{k: t[k] for k in ("shs", "colors_precomp", "scales", "rotations") if k in t})
    rgb, wm = res[0], res[1]
    assert wm.stride() == (1, 192 * 96, 192) and tuple(rgb.shape) == (3, 80, 96)
    np.testing.assert_array_equal(wm.cpu().numpy(), ref_f["lang"])
    g = np.random.default_rng(3)
    cb = g.standard_normal((L, K, DF)).astype(F32)
    e = mixed_prompt(g, cb)
    ref, n = ref_summed(ref_f["lang"], cb, e)
    print(f"float64 summed cosine on the render: min {ref.min():.4f} max {ref.max():.4f} min |s| "
          f"{n[n > 0].min():.3f}")
    assert ref.max() >= 0.22 and ref.max() - ref.min() >= 0.02
    assert n[n > 0].min() >= 1.0
    maps = heatmap.summed_similarity_maps(wm, to_gpu(cb, gpu), to_gpu(e, gpu))
    check(maps, ref, HEAT_ATOL, "render + summed cosine")
    lut = heatmap.jet_lut(gpu)
    got = heatmap.heat_frames(maps, lut, rgb=rgb)
    want = np_heat_frames(maps.cpu().numpy(), lut.cpu().numpy(), rgb.contiguous().cpu().numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.gpu
def test_plan_cache(gpu):
    g = np.random.default_rng(6)
    wmap, cbn, posn, negn = sparse_map(g, 16, 24, 0.2), g.standard_normal((L, K, DF)).astype(F32), unit(g, 3), unit(g, 4)
    wm, cb, pos, neg = (to_gpu(a, gpu) for a in (wmap, cbn, posn, negn))
    p0 = heatmap.heat_plan(cb, pos, neg)
    a = heatmap.mean_relevancy_maps(wm, cb, pos, neg)
    assert heatmap.heat_plan(cb, pos, neg) is p0                          # the same prompt across frames
    assert heatmap.heat_plan(cb, pos) is not p0                           # without negatives: another plan
    assert torch.equal(a, heatmap.mean_relevancy_maps(wm, cb, pos, neg))
    s0 = heatmap.summed_similarity_maps(wm, cb, pos)
    assert torch.equal(s0, heatmap.summed_similarity_maps(wm, cb, pos))
    cb.mul_(-0.5)                                                          # in place: the version counter moves
    assert heatmap.heat_plan(cb, pos, neg) is not p0
    check(heatmap.mean_relevancy_maps(wm, cb, pos, neg), ref_mean_relevancy(wmap, cb.cpu().numpy(), posn, negn),
          REL_ATOL, "after codebook update")
    check(heatmap.summed_similarity_maps(wm, cb, pos), ref_summed(wmap, cb.cpu().numpy(), posn)[0], HEAT_ATOL,
          "summed cosine after codebook update")
    p1 = heatmap.heat_plan(cb, pos)
    pos2n = unit(g, 3)
    pos2 = to_gpu(pos2n, gpu)                                              # a new prompt
    assert heatmap.heat_plan(cb, pos2) is not p1
    check(heatmap.summed_similarity_maps(wm, cb, pos2), ref_summed(wmap, cb.cpu().numpy(), pos2n)[0], HEAT_ATOL,
          "new prompt")
    # fp16 embeddings (the reference's dtype): cast to fp32 and used as given
    ph = pos2.half()
    check(heatmap.summed_similarity_maps(wm, cb, ph),
          ref_summed(wmap, cb.cpu().numpy(), ph.float().cpu().numpy())[0], HEAT_ATOL, "fp16 embeddings")
    assert heatmap.heat_plan(cb, ph) is heatmap.heat_plan(cb, ph)
    # the query module's plans are separate buffers of their own size
    assert query.query_plan(cb, pos, neg).buf.numel() == _lib.load().lsr_quick_query_plan_bytes(L, K, DF, 3, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("demo", [False, True], ids=["server", "demo"])
def test_heat_stream(gpu, demo):
    """QuickHeatStream over 3 pushed (map, rgb) pairs equals the direct calls
    bit for bit, from the default stream and from inside a non-default caller
    stream."""
    g = np.random.default_rng(9)
    H, W = 33, 52
    maps = [to_gpu(sparse_map(g, H, W), gpu, hwc=bool(i & 1)) for i in range(3)]
    rgbs = [to_gpu(g.random((3, H, W)).astype(F32), gpu) for _ in range(3)]
    cbn = g.standard_normal((L, K, DF)).astype(F32)
    cb, pos, neg = to_gpu(cbn, gpu), to_gpu(np.concatenate([mixed_prompt(g, cbn), unit(g, 2)]), gpu), to_gpu(unit(g, 4), gpu)
    lut = heatmap.jet_lut(gpu)
    if demo:
        kw = dict(curve="power4", min_range=0.0)
        ref = [heatmap.heat_frames(heatmap.mean_relevancy_maps(m, cb, pos, neg), lut, **kw) for m in maps]
    else:
        kw = dict(threshold=0.2)
        ref = [heatmap.heat_frames(heatmap.summed_similarity_maps(m, cb, pos), lut, rgb=r, **kw)
               for m, r in zip(maps, rgbs)]
    torch.cuda.synchronize()
    assert len(torch.unique(ref[0][0].reshape(-1, 3), dim=0)) > 16        # the first prompt's frame is live

    def run():
        hs = heatmap.QuickHeatStream(cb, pos, lut, neg_embeds=neg if demo else None, **kw)
        got = [hs.push(lambda m=m, r=r: (m, None if demo else r)) for m, r in zip(maps, rgbs)]
        assert got[0] is None
        got = got[1:] + [hs.flush()]
        assert hs.flush() is None
        return got

    got = run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        got = run()
        sums = torch.stack([o.double().sum() for o in got])               # used on the caller's stream, no sync
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert torch.equal(sums, torch.stack([r.double().sum() for r in ref]))
