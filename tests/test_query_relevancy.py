"""Fused text-query relevancy / cosine maps of the quick path
(langsplatv2_amd.query, csrc/quick_query.hip k_quick_query) against the reference's
OpenCLIPNetwork.get_max_across_quick (eval/openclip_encoder.py:114-139) applied
to the float64 decode of the weight map (eval_lerf.py:214-218).

tests/golden/ref_relevancy.npz holds the reference function's own float64
output on a seeded fixture (make_ref_relevancy.py); `ref_relevancy` below is
this file's numpy-float64 restatement, pinned to it within 1e-12 and used for
every other shape.

Tolerances (derived, not fitted): the project holds normalised decode outputs
to 1e-6 absolute on values in [-1, 1] (test_quick_decode.DEC_ATOL); a cosine
similarity is the dot product of that unit vector with a unit vector, so
similarity_maps is held to SIM_ATOL = 1e-6 absolute.  Relevancy is
sigmoid(10 d) with d = sim_pos - max sim_neg: |delta d| <= 2e-6 and
|d sigmoid(10 d) / dd| <= 2.5, so REL_ATOL = 5e-6 absolute (inside the
north star's 1e-5).  The reference's own fp32 evaluation deviates 2.2e-7 from
float64 on the fixture (ref_fp32_max_dev in the .npz).
Measured on the MI355X over this file's cases: relevancy <= 1.5e-7, similarity
<= 7.2e-8 ("Fused text-query relevancy").
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from langsplatv2_amd import _lib, query
from test_quick_decode import ref_decode

SIM_ATOL = 1e-6
REL_ATOL = 5e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_relevancy.npz")
L, K, DF = 3, 64, 512


def ref_similarity(wmap, cb, embeds, eps=1e-10):
    """(L, Q, H, W) float64: the normalised decode dotted with each embedding."""
    F = ref_decode(wmap, cb, True, eps)                                   # (L, Df, H, W)
    return np.einsum("ldhw,qd->lqhw", F, embeds.astype(np.float64))


def ref_relevancy(wmap, cb, pos, neg, scale=10.0, eps=1e-10):
    """get_max_across_quick in numpy float64: for every positive the 2-way
    softmax against each negative, then the minimum of the positive's share."""
    sp = ref_similarity(wmap, cb, pos, eps)[:, :, None]                   # (L, Q, 1, H, W)
    sn = ref_similarity(wmap, cb, neg, eps)[:, None]                      # (L, 1, N, H, W)
    a, b = np.broadcast_arrays(scale * sp, scale * sn)
    m = np.maximum(a, b)
    ea, eb = np.exp(a - m), np.exp(b - m)
    return (ea / (ea + eb)).min(axis=2)


def unit(g, n, d=DF):
    e = g.standard_normal((n, d))
    return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)


def sparse_map(g, H, W, density=0.15):
    return (g.random((L * K, H, W)) * (g.random((L * K, H, W)) < density)).astype(np.float32)


def to_gpu(a, gpu, hwc=False):
    t = torch.tensor(np.asarray(a)).to(gpu)   # (a copy: the shared cases are read-only)
    if hwc:   # the rasterizer's pixel-major buffer, seen as (D, H, W)
        t = t.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    return t


def check(got, ref, atol, name):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), name
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{name}: max abs err {err:.3e} (bound {atol:g})")
    assert err <= atol, f"{name}: max abs err {err:.3e} > {atol:g}"


@functools.lru_cache(maxsize=None)
def case(H, W, Q, N):
    """Seeded inputs and float64 references of one shape, shared by the tests (read only)."""
    g = np.random.default_rng(H * 100000 + W * 100 + Q * 7 + N)
    wmap, cb, pos, neg = sparse_map(g, H, W), g.standard_normal((L, K, DF)).astype(np.float32), unit(g, Q), unit(g, N)
    out = dict(wmap=wmap, cb=cb, pos=pos, neg=neg, rel=ref_relevancy(wmap, cb, pos, neg),
               sim=ref_similarity(wmap, cb, pos))
    for v in out.values():
        v.setflags(write=False)
    return out


SHAPES = [(37, 45), (64, 128), (1, 1)]          # W no multiple of 4 or 64; an exact tile; a single pixel
QUERIES = [(1, 4), (13, 4), (3, 20)]            # the reference's default; positives / negatives crossing a 16-column block


# ---------------------------------------------------------------- CPU

def test_restatement_matches_reference_golden():
    z = np.load(GOLDEN)
    got = ref_relevancy(z["weight_map"], z["codebooks"], z["pos_embeds"], z["neg_embeds"])
    assert got.shape == z["relevancy"].shape == (3, 3, 12, 20)
    assert np.abs(got - z["relevancy"]).max() <= 1e-12
    assert float(z["ref_fp32_max_dev"]) < 1e-6
    y, x = z["zero_pixel"]
    assert not z["weight_map"][:, y, x].any() and np.all(z["relevancy"][:, :, y, x] == 0.5)


def test_validation_on_cpu():
    wm, cb, pos, neg = torch.zeros(192, 4, 4), torch.zeros(3, 64, 512), torch.zeros(2, 512), torch.zeros(4, 512)
    with pytest.raises(ValueError):
        query.relevancy_maps(torch.zeros(4, 4), cb, pos, neg)             # rank
    with pytest.raises(ValueError):
        query.relevancy_maps(wm, torch.zeros(64, 512), pos, neg)
    with pytest.raises(ValueError):
        query.relevancy_maps(wm, cb, torch.zeros(512), neg)
    with pytest.raises(ValueError):
        query.relevancy_maps(torch.zeros(100, 4, 4), cb, pos, neg)        # channels != L*K
    with pytest.raises(ValueError):
        query.relevancy_maps(wm, cb, torch.zeros(2, 256), neg)            # embedding width != Df
    with pytest.raises(ValueError):
        query.relevancy_maps(wm, cb, pos, torch.zeros(4, 500))
    with pytest.raises(ValueError):
        query.similarity_maps(wm, cb, torch.zeros(2, 256))
    with pytest.raises(ValueError):
        query.similarity_maps(torch.zeros(100, 4, 4), cb, pos)
    with pytest.raises(RuntimeError, match="no CPU path"):
        query.relevancy_maps(wm, cb, pos, neg)
    with pytest.raises(RuntimeError, match="no CPU path"):
        query.similarity_maps(wm, cb, pos)
    with pytest.raises(RuntimeError, match="no CPU path"):
        query.query_plan(cb, pos, neg)


def test_abi_status_codes_without_device():
    lib = _lib.load()
    f = ctypes.c_float
    assert lib.lsr_quick_query_plan_bytes(3, 48, 512, 3, 4) == 0
    assert lib.lsr_quick_query_plan_bytes(3, 64, 500, 3, 4) == 0
    assert lib.lsr_quick_query_plan_bytes(3, 64, 512, 61, 4) == 0
    assert lib.lsr_quick_query_plan_bytes(3, 64, 512, 3, 4) >= 3 * (1 + 4) * 4096
    assert lib.lsr_quick_query_plan_bytes(3, 64, 512, 4, 4) == 172544   # the plan's size is part of the ABI
    run = lib.lsr_quick_query_run
    assert run(None, 0, None, 3, 64, 3, 4, 8, 8, 0, f(10), f(1e-10), None, None) == 1        # null map
    assert run(None, 2, None, 3, 64, 3, 4, 8, 8, 0, f(10), f(1e-10), None, None) == 1        # no such layout
    assert run(None, 0, None, 3, 64, 3, 4, 8, 8, 2, f(10), f(1e-10), None, None) == 1        # no such mode
    assert run(None, 0, None, 3, 64, 61, 4, 8, 8, 0, f(10), f(1e-10), None, None) == 2       # n_pos + n_neg > 64
    assert run(None, 0, None, 3, 48, 3, 4, 8, 8, 0, f(10), f(1e-10), None, None) == 2        # K != 64
    assert run(None, 0, None, 3, 64, 3, 0, 8, 8, 0, f(10), f(1e-10), None, None) == 2        # relevancy, no negatives
    assert run(None, 0, None, 3, 64, 3, 4, 0, 8, 0, f(10), f(1e-10), None, None) == 0        # H = 0
    assert run(None, 0, None, 0, 64, 3, 0, 8, 8, 1, f(0), f(1e-10), None, None) == 0         # L = 0
    prep = lib.lsr_quick_query_prepare
    assert prep(None, None, None, 3, 64, 512, 3, 4, None, None) == 1
    assert prep(None, None, None, 3, 64, 512, 0, 4, None, None) == 1
    assert prep(None, None, None, 3, 64, 512, 61, 4, None, None) == 2


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_golden(gpu):
    z = np.load(GOLDEN)
    got = query.relevancy_maps(*(to_gpu(z[k], gpu) for k in ("weight_map", "codebooks", "pos_embeds", "neg_embeds")))
    check(got, z["relevancy"], REL_ATOL, "golden relevancy")
    y, x = z["zero_pixel"]
    assert torch.all(got[:, :, y, x] == 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
@pytest.mark.parametrize("Q,N", QUERIES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_relevancy_matches_float64(gpu, H, W, Q, N, hwc):
    c = case(H, W, Q, N)
    wm = to_gpu(c["wmap"], gpu, hwc)
    if hwc and H * W > 1:
        assert wm.stride() == (1, L * K * W, L * K)
    got = query.relevancy_maps(wm, to_gpu(c["cb"], gpu), to_gpu(c["pos"], gpu), to_gpu(c["neg"], gpu))
    check(got, c["rel"], REL_ATOL, f"relevancy {H}x{W} Q={Q} N={N} {'hwc' if hwc else 'chw'}")


@pytest.mark.gpu
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
@pytest.mark.parametrize("Q,N", QUERIES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_similarity_matches_float64(gpu, H, W, Q, N, hwc):
    c = case(H, W, Q, N)
    got = query.similarity_maps(to_gpu(c["wmap"], gpu, hwc), to_gpu(c["cb"], gpu), to_gpu(c["pos"], gpu))
    check(got, c["sim"], SIM_ATOL, f"similarity {H}x{W} Q={Q} {'hwc' if hwc else 'chw'}")


@pytest.mark.gpu
def test_chunked_positives_equal_their_chunks(gpu):
    """Q = 70 with 4 negatives: 60 + 10 positives in two launches, each chunk's
    planes bit for bit those of a call with that chunk alone."""
    g = np.random.default_rng(70)
    wm, cb = to_gpu(sparse_map(g, 21, 36), gpu), to_gpu(g.standard_normal((L, K, DF)).astype(np.float32), gpu)
    pos, neg = to_gpu(unit(g, 70), gpu), to_gpu(unit(g, 4), gpu)
    got = query.relevancy_maps(wm, cb, pos, neg)
    assert got.shape == (L, 70, 21, 36)
    assert torch.equal(got[:, :60], query.relevancy_maps(wm, cb, pos[:60].clone(), neg))
    assert torch.equal(got[:, 60:], query.relevancy_maps(wm, cb, pos[60:].clone(), neg))
    check(got, ref_relevancy(*(t.cpu().numpy() for t in (wm, cb, pos, neg))), REL_ATOL, "relevancy Q=70")


@pytest.mark.gpu
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
def test_special_pixels(gpu, hwc):
    """An all-zero pixel gives relevancy 0.5 and similarity 0 exactly (the
    reference: 0 / (0 + 1e-10)); pixels scaled by 1e-12 (|f| comparable to
    eps), 1e-20, 1e-30 and 1e-40 (subnormal) stay finite and within tolerance;
    every other pixel keeps the bits it has without them."""
    g = np.random.default_rng(12)
    H, W = 24, 40
    base = sparse_map(g, H, W, 0.2)
    wmap = base.copy()
    special = {(0, 0): 1e-40, (7, 9): 1e-30, (11, 20): 1e-20, (23, 39): 1e-12, (5, 17): 0.0}
    for (y, x), s in special.items():
        wmap[:, y, x] = (wmap[:, y, x].astype(np.float64) * s).astype(np.float32)
    cb, pos, neg = g.standard_normal((L, K, DF)).astype(np.float32), unit(g, 3), unit(g, 4)
    t = [to_gpu(a, gpu) for a in (cb, pos, neg)]
    rel = query.relevancy_maps(to_gpu(wmap, gpu, hwc), *t)
    sim = query.similarity_maps(to_gpu(wmap, gpu, hwc), t[0], t[1])
    check(rel, ref_relevancy(wmap, cb, pos, neg), REL_ATOL, "special pixels relevancy")
    check(sim, ref_similarity(wmap, cb, pos), SIM_ATOL, "special pixels similarity")
    assert torch.all(rel[:, :, 5, 17] == 0.5) and torch.all(sim[:, :, 5, 17] == 0.0)
    keep = torch.ones(H, W, dtype=torch.bool, device=gpu)
    for (y, x) in special:
        keep[y, x] = False
    rel0 = query.relevancy_maps(to_gpu(base, gpu, hwc), *t)
    sim0 = query.similarity_maps(to_gpu(base, gpu, hwc), t[0], t[1])
    assert torch.equal(rel[:, :, keep], rel0[:, :, keep]) and torch.equal(sim[:, :, keep], sim0[:, :, keep])


@pytest.mark.gpu
def test_rank_deficient_codebook(gpu):
    """Duplicated codes (a singular Gram matrix, as in
    test_quick_decode.test_plan_reuse_one_shot_and_invalidation)."""
    g = np.random.default_rng(5)
    wmap, cb, pos, neg = sparse_map(g, 20, 28, 0.2), g.standard_normal((L, K, DF)).astype(np.float32), unit(g, 3), unit(g, 4)
    cb[:, 32:] = cb[:, :32]
    t = [to_gpu(a, gpu) for a in (wmap, cb, pos, neg)]
    check(query.relevancy_maps(*t), ref_relevancy(wmap, cb, pos, neg), REL_ATOL, "rank-32 codebook relevancy")
    check(query.similarity_maps(*t[:3]), ref_similarity(wmap, cb, pos), SIM_ATOL, "rank-32 codebook similarity")


@pytest.mark.gpu
def test_plan_cache(gpu):
    g = np.random.default_rng(6)
    wmap, cbn, posn, negn = sparse_map(g, 16, 24, 0.2), g.standard_normal((L, K, DF)).astype(np.float32), unit(g, 3), unit(g, 4)
    wm, cb, pos, neg = (to_gpu(a, gpu) for a in (wmap, cbn, posn, negn))
    p0 = query.query_plan(cb, pos, neg)
    a = query.relevancy_maps(wm, cb, pos, neg)
    assert query.query_plan(cb, pos, neg) is p0                           # the same prompt across frames
    assert torch.equal(a, query.relevancy_maps(wm, cb, pos, neg))
    cb.mul_(-0.5)                                                          # in place: the version counter moves
    assert query.query_plan(cb, pos, neg) is not p0
    check(query.relevancy_maps(wm, cb, pos, neg), ref_relevancy(wmap, cb.cpu().numpy(), posn, negn), REL_ATOL,
          "after codebook update")
    p1 = query.query_plan(cb, pos, neg)
    pos2n = unit(g, 3)
    pos2 = to_gpu(pos2n, gpu)                                              # a new prompt
    assert query.query_plan(cb, pos2, neg) is not p1
    check(query.relevancy_maps(wm, cb, pos2, neg), ref_relevancy(wmap, cb.cpu().numpy(), pos2n, negn), REL_ATOL,
          "new prompt")
    # fp16 embeddings (the reference's dtype): cast to fp32 and used as given
    ph, nh = pos2.half(), neg.half()
    check(query.relevancy_maps(wm, cb, ph, nh),
          ref_relevancy(wmap, cb.cpu().numpy(), ph.float().cpu().numpy(), nh.float().cpu().numpy()), REL_ATOL,
          "fp16 embeddings")
    assert query.query_plan(cb, ph, nh) is query.query_plan(cb, ph, nh)


@pytest.mark.gpu
def test_relevancy_stream(gpu):
    """QuickRelevancyStream over 3 pushed maps equals the direct calls bit for
    bit, from the default stream and from inside a non-default caller stream."""
    g = np.random.default_rng(9)
    maps = [to_gpu(sparse_map(g, 33, 52), gpu, hwc=bool(i & 1)) for i in range(3)]
    cb = to_gpu(g.standard_normal((L, K, DF)).astype(np.float32), gpu)
    pos, neg = to_gpu(unit(g, 3), gpu), to_gpu(unit(g, 4), gpu)
    ref = [query.relevancy_maps(m, cb, pos, neg) for m in maps]
    torch.cuda.synchronize()

    def run():
        rs = query.QuickRelevancyStream(cb, pos, neg)
        got = [rs.push(lambda m=m: m) for m in maps]
        assert got[0] is None
        got = got[1:] + [rs.flush()]
        assert rs.flush() is None
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


@pytest.mark.gpu
def test_render_then_relevancy_end_to_end(gpu, oracle_lib):
    """Quick render through the drop-in rasterizer at its default (pixel-major)
    layout, then relevancy_maps, vs the restatement on the oracle's weight map."""
    from harness import make_case, oracle_problem
    from test_quick_stream import _renderer
    case_ = make_case(N=3000, W=96, H=80, seed=21, sh_degree=None, quick_k=4)
    ref_f = oracle_lib.forward(oracle_problem(case_))
    wm = _renderer(case_, gpu, None)()
    assert wm.stride() == (1, 192 * 96, 192)                               # the default layout is pixel-major
    np.testing.assert_array_equal(wm.cpu().numpy(), ref_f["lang"])
    g = np.random.default_rng(3)
    cb, pos, neg = g.standard_normal((L, K, DF)).astype(np.float32), unit(g, 3), unit(g, 4)
    got = query.relevancy_maps(wm, *(to_gpu(a, gpu) for a in (cb, pos, neg)))
    check(got, ref_relevancy(ref_f["lang"], cb, pos, neg), REL_ATOL, "render + relevancy")
