"""Parity of the HIP path (through the C ABI / drop-in surface) against the
oracle.  Forward outputs and all index work are compared BIT-EXACTLY; the
backward within the tolerance in tests/harness.py (fp32 sums in a different
order).  Runs on the GPU box: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from harness import (assert_grad_close, assert_img, fwd_atol, make_case, oracle_problem, run_gpu_fwd_bwd,
                     run_gpu_forward)

pytestmark = pytest.mark.gpu

CASES = {
    # name: make_case kwargs
    "cfg1_rgb": dict(N=1000, W=128, H=128, sh_degree=None),
    "sh3_lang16_ragged": dict(N=10000, W=250, H=190, sh_degree=3, lang_dim=16, bg=(0.3, 0.6, 1.0), seed=3),
    "rgb_lang3": dict(N=8000, W=200, H=120, sh_degree=None, lang_dim=3, seed=4),
    "cov_precomp_lang8": dict(N=6000, W=160, H=96, sh_degree=2, lang_dim=8, cov_precomp=True, seed=5),
    "sh1_scalemod": dict(N=5000, W=144, H=144, sh_degree=1, scale_modifier=1.3, seed=6),
    "lang64_feature_mode": dict(N=4000, W=128, H=112, sh_degree=3, lang_dim=64, seed=7),
    "yaw_sh3_lang32": dict(N=8000, W=192, H=128, sh_degree=3, lang_dim=32, yaw=15.0, seed=8),
    "quick192": dict(N=5000, W=128, H=96, sh_degree=None, quick_k=4, seed=9),
    # language widths below their compiled set (32, 64): the forward's MFMA
    # language blocks mask the channels past D
    "sh2_lang24_ragged": dict(N=6000, W=136, H=100, sh_degree=2, lang_dim=24, bg=(0.2, 0.1, 0.7), seed=10),
    "lang48": dict(N=4000, W=112, H=96, sh_degree=3, lang_dim=48, seed=11),
    # and below the 16-channel set: the masked D = 16 forward, the D < 16 backward over set 16
    "lang12": dict(N=3000, W=96, H=80, sh_degree=2, lang_dim=12, seed=12),
}


def _fwd_compare(case, gpu, oracle_lib, grad_request=0):
    """grad_request: see harness.run_gpu_forward (0: the inference forward)."""
    pb = oracle_problem(case)
    ref = oracle_lib.forward(pb)
    got = run_gpu_forward(case, gpu, grad_request=grad_request)
    vis = ref["radii"] > 0
    np.testing.assert_array_equal(got["radii"], ref["radii"])
    np.testing.assert_array_equal(got["tiles_touched"], ref["tiles_touched"].astype(np.int32))
    assert got["num_rendered"] == ref["num_rendered"]
    np.testing.assert_array_equal(got["xy"][vis], ref["xy"][vis])
    np.testing.assert_array_equal(got["conic_opacity"][vis], ref["conic_opacity"][vis])
    np.testing.assert_array_equal(got["depth"][vis], ref["depth"][vis])
    if case["g"].get("shs") is not None:
        np.testing.assert_array_equal(got["rgb"][vis], ref["rgb"][vis])
    # index work: per-tile ranges and depth-ordered lists
    np.testing.assert_array_equal(got["ranges"], ref["ranges"].astype(np.int32))
    np.testing.assert_array_equal(got["point_list"], ref["point_list"].astype(np.int32))
    # image outputs
    np.testing.assert_array_equal(got["n_contrib"], ref["n_contrib"].astype(np.int32))
    fa = fwd_atol(case)
    assert_img(got["final_T"], ref["final_T"], fa, "final_T")
    assert_img(got["color"], ref["color"], fa, "color")
    assert_img(got["lang"], ref["lang"], fa, "lang")
    return ref, got


@pytest.mark.parametrize("name", list(CASES))
def test_forward_bit_exact(name, gpu, oracle_lib):
    case = make_case(**CASES[name])
    _fwd_compare(case, gpu, oracle_lib)


@pytest.mark.parametrize("name", [n for n in CASES if n != "quick192"] + ["quick192"])
def test_backward_vs_oracle(name, gpu, oracle_lib):
    case = make_case(**CASES[name])
    pb = oracle_problem(case)
    ref = oracle_lib.forward(pb)
    rng = np.random.default_rng(1)
    H, W = case["cam"]["H"], case["cam"]["W"]
    dcol = rng.standard_normal((3, H, W)).astype(np.float32)
    dlang = rng.standard_normal((pb.D, H, W)).astype(np.float32) if pb.D else None
    rb = oracle_lib.backward(pb, ref, dcol, dlang)
    got = run_gpu_fwd_bwd(case, gpu, dcol, dlang)
    assert_img(got["color"], ref["color"], fwd_atol(case), "color")
    assert_grad_close("means2D", got["grad_means2D"], rb["dmean2D"])
    assert_grad_close("opacities", got["grad_opacities"], rb["dopacity"][:, None])
    assert_grad_close("means3D", got["grad_means3D"], rb["dmeans3D"])
    if "grad_colors_precomp" in got:
        assert_grad_close("colors_precomp", got["grad_colors_precomp"], rb["dcolor"])
    if "grad_shs" in got:
        assert_grad_close("shs", got["grad_shs"], rb["dsh"])
    if "grad_scales" in got:
        assert_grad_close("scales", got["grad_scales"], rb["dscales"])
        assert_grad_close("rotations", got["grad_rotations"], rb["drot"])
    if "grad_cov3D_precomp" in got:
        assert_grad_close("cov3D_precomp", got["grad_cov3D_precomp"], rb["dcov3D"])
    if pb.D:
        assert_grad_close("language_feature_precomp", got["grad_language_feature_precomp"], rb["dlang"])


@pytest.mark.parametrize("N", [1, 5, 16, 23, 40, 70])
def test_block_list_chunk_boundaries(N, gpu, oracle_lib):
    """One 16x16 tile (four 8x8 blocks) at D = 16: the backward reads each
    block's candidate list in chunks of one 16-candidate group
    (render_bwd.hip LSR_LST_CHUNK) with a counted DMA wait, so list lengths below,
    at and across multiples of 16 (and a lone candidate) must give the
    oracle's gradients."""
    case = make_case(N=N, W=16, H=16, sh_degree=None, lang_dim=16, seed=40 + N)
    pb = oracle_problem(case)
    ref = oracle_lib.forward(pb)
    rng = np.random.default_rng(2)
    dcol = rng.standard_normal((3, 16, 16)).astype(np.float32)
    dlang = rng.standard_normal((16, 16, 16)).astype(np.float32)
    rb = oracle_lib.backward(pb, ref, dcol, dlang)
    got = run_gpu_fwd_bwd(case, gpu, dcol, dlang)
    assert_img(got["color"], ref["color"], fwd_atol(case), "color")
    assert_grad_close("means2D", got["grad_means2D"], rb["dmean2D"])
    assert_grad_close("opacities", got["grad_opacities"], rb["dopacity"][:, None])
    assert_grad_close("colors_precomp", got["grad_colors_precomp"], rb["dcolor"])
    assert_grad_close("language_feature_precomp", got["grad_language_feature_precomp"], rb["dlang"])


@pytest.mark.parametrize("name", ["sh3_lang16_ragged", "rgb_lang3", "cov_precomp_lang8", "lang64_feature_mode",
                                  "yaw_sh3_lang32"])
def test_language_only_backward(name, gpu, oracle_lib):
    """Feature-mode autograd: only the language input requires grad (geometry
    frozen, scene/gaussian_model.py:238-243; means2D without grad), so the
    library runs its language-only backward.  dL/dlanguage vs the oracle."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from harness import settings_for
    case = make_case(**CASES[name])
    pb = oracle_problem(case)
    ref = oracle_lib.forward(pb)
    rng = np.random.default_rng(1)
    H, W = case["cam"]["H"], case["cam"]["W"]
    dcol = rng.standard_normal((3, H, W)).astype(np.float32)
    dlang = rng.standard_normal((pb.D, H, W)).astype(np.float32)
    rb = oracle_lib.backward(pb, ref, dcol, dlang)
    t = {k: v.to(gpu) for k, v in case["g"].items() if isinstance(v, torch.Tensor)}
    lang = t["language_feature_precomp"].clone().requires_grad_(True)
    kw = {k: t[k] for k in ("shs", "colors_precomp", "scales", "rotations", "cov3D_precomp") if k in t}
    r = GaussianRasterizer(settings_for(case, gpu))
    color, lo, _ = r(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"],
                     language_feature_precomp=lang, **kw)
    torch.autograd.backward([color, lo], [torch.from_numpy(dcol).to(gpu), torch.from_numpy(dlang).to(gpu)])
    assert_img(lo.detach().cpu().numpy(), ref["lang"], fwd_atol(case), "lang")
    assert_grad_close("language_feature_precomp", lang.grad.cpu().numpy(), rb["dlang"])


def test_empty_and_all_culled(gpu, oracle_lib):
    for N, behind in ((0, False), (300, True)):
        case = make_case(N=max(N, 1) if N else 0, W=64, H=48, sh_degree=None, seed=11) if N else None
        if N == 0:
            case = make_case(N=10, W=64, H=48, sh_degree=None, seed=11)
            for k, v in list(case["g"].items()):
                if isinstance(v, torch.Tensor):
                    case["g"][k] = v[:0].contiguous()
        else:
            case = make_case(N=N, W=64, H=48, sh_degree=None, seed=11)
            case["g"]["means3D"][:, 2] = -1.0  # all behind the near plane
        case["bg"] = (0.25, 0.5, 0.75)
        ref, got = _fwd_compare(case, gpu, oracle_lib)
        assert got["num_rendered"] == 0
        np.testing.assert_array_equal(got["color"][0], np.full((48, 64), 0.25, np.float32))


def test_big_tile_global_sort(gpu, oracle_lib):
    """> 4096 instances in some tiles exercises the chunked LDS + global merge path."""
    case = make_case(N=26000, W=48, H=32, sh_degree=None, seed=12)
    ref, got = _fwd_compare(case, gpu, oracle_lib)
    counts = ref["ranges"][:, 1] - ref["ranges"][:, 0]
    assert counts.max() > 4096, counts.max()


@pytest.mark.parametrize("N,W,H,lo,hi", [(4000, 48, 32, 512, 1024), (14000, 64, 48, 1024, 2048)])
def test_tile_sort_size_classes(gpu, oracle_lib, N, W, H, lo, hi):
    """Tiles of 513-1024 instances (class 0: one wave, up to 16 keys per lane)
    and of 1025-2048 (class 1: a 4-wave workgroup, 8 keys per lane): bit-exact lists."""
    case = make_case(N=N, W=W, H=H, sh_degree=None, seed=12)
    ref, got = _fwd_compare(case, gpu, oracle_lib)
    counts = ref["ranges"][:, 1] - ref["ranges"][:, 0]
    assert counts.min() > lo and counts.max() <= hi, (counts.min(), counts.max())


def test_forward_deterministic(gpu):
    case = make_case(**CASES["sh3_lang16_ragged"])
    a = run_gpu_forward(case, gpu)
    b = run_gpu_forward(case, gpu)
    for k in ("color", "lang", "point_list", "n_contrib", "final_T"):
        np.testing.assert_array_equal(a[k], b[k])


def test_mark_visible(gpu):
    from diff_gaussian_rasterization import GaussianRasterizer
    from harness import settings_for
    case = make_case(N=2000, W=64, H=64, sh_degree=None, seed=13)
    rs = settings_for(case, gpu)
    vis = GaussianRasterizer(rs).markVisible(case["g"]["means3D"].to(gpu)).cpu().numpy()
    m = case["g"]["means3D"].numpy()
    np.testing.assert_array_equal(vis, m[:, 2] > 0.2)


def test_input_validation(gpu):
    from diff_gaussian_rasterization import GaussianRasterizer
    from harness import settings_for
    case = make_case(N=100, W=32, H=32, sh_degree=None, seed=14)
    rs = settings_for(case, gpu)
    t = {k: v.to(gpu) for k, v in case["g"].items() if isinstance(v, torch.Tensor)}
    r = GaussianRasterizer(rs)
    with pytest.raises(Exception, match="one of either SHs"):
        r(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"],
          scales=t["scales"], rotations=t["rotations"])
    with pytest.raises(Exception, match="scale/rotation pair"):
        r(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"],
          colors_precomp=t["colors_precomp"], scales=t["scales"])
    with pytest.raises(RuntimeError, match="ROCm device"):
        r(means3D=t["means3D"].cpu(), means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"],
          colors_precomp=t["colors_precomp"], scales=t["scales"], rotations=t["rotations"])


def test_global_atomic_binning_fallback(gpu, oracle_lib):
    """Images wider than the privatised binning's LDS band (gx * 4 B > 32 KB,
    i.e. > 8192 tiles per row) bin through the global-atomic pair k_duplicate /
    k_scatter (binning.hip; lsr_api.hip `priv`).  VERDICT r03 asked for it to be
    tested or removed: 131,200 x 32 px (8,200 x 2 tiles), the whole binning and
    48 sampled tiles' images bit-exact against the oracle."""
    W, H = 16 * 8200, 32
    case = make_case(N=3000, W=W, H=H, sh_degree=None, seed=15)
    gx = (W + 15) // 16
    assert gx * 4 > 32768
    tiles = np.sort(np.random.default_rng(2).choice(gx * 2, size=48, replace=False)).astype(np.int32)
    pb = oracle_problem(case)
    ref = oracle_lib.forward(pb, nthreads=8, tiles=tiles)
    got = run_gpu_forward(case, gpu)
    # this path sizes its workspace before the cull (its per-instance rank
    # array covers every rect instance), so num_rendered is the rect total --
    # the reference's own num_rendered -- while the ranges / lists hold the
    # culled instances: the first ranges[-1] entries are the oracle's list
    m = int(ref["num_rendered"])
    assert got["num_rendered"] >= m > 10000
    np.testing.assert_array_equal(got["radii"], ref["radii"])
    np.testing.assert_array_equal(got["ranges"], ref["ranges"].astype(np.int32))
    assert int(got["ranges"][:, 1].max()) == m
    np.testing.assert_array_equal(got["point_list"][:m], ref["point_list"].astype(np.int32))
    for t in tiles:
        tx, ty = t % gx, t // gx
        sl = (slice(ty * 16, ty * 16 + 16), slice(tx * 16, tx * 16 + 16))
        assert_img(got["color"][(slice(None),) + sl], ref["color"][(slice(None),) + sl], fwd_atol(case), "color")
        assert_img(got["final_T"][sl], ref["final_T"][sl], fwd_atol(case), "final_T")
        np.testing.assert_array_equal(got["n_contrib"][sl], ref["n_contrib"][sl].astype(np.int32))


@pytest.mark.parametrize("name", ["sh3_lang16_ragged", "yaw_sh3_lang32", "lang64_feature_mode", "cfg1_rgb"])
def test_backward_without_block_lists(name, gpu, oracle_lib):
    """The backward re-stages its candidates from the tile lists when the
    forward's per-block candidate lists are absent (a host that does not pass
    lsr_fwd_out.lists back): same gradients as the list path and the oracle."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from harness import gpu_inputs, settings_for
    case = make_case(**CASES[name])
    pb = oracle_problem(case)
    ref = oracle_lib.forward(pb)
    rng = np.random.default_rng(1)
    H, W = case["cam"]["H"], case["cam"]["W"]
    dcol = rng.standard_normal((3, H, W)).astype(np.float32)
    dlang = rng.standard_normal((pb.D, H, W)).astype(np.float32) if pb.D else None
    rb = oracle_lib.backward(pb, ref, dcol, dlang)
    from langsplatv2_amd import _lib
    t = gpu_inputs(case, gpu, requires_grad=True)
    kw = {k: t[k] for k in ("shs", "colors_precomp", "scales", "rotations", "language_feature_precomp") if k in t}
    prev = _lib.set_lists_max_mb(0)          # no budget: the forward writes no block lists
    try:
        color, lang, _ = GaussianRasterizer(settings_for(case, gpu))(means3D=t["means3D"], means2D=t["means2D"],
                                                                     opacities=t["opacities"], **kw)
    finally:
        _lib.set_lists_max_mb(prev)
    assert color.grad_fn.saved_tensors[-1] is None   # ... so the backward re-stages
    outs, grads = [color], [torch.from_numpy(dcol).to(gpu)]
    if pb.D:
        outs.append(lang)
        grads.append(torch.from_numpy(dlang).to(gpu))
    torch.autograd.backward(outs, grads)
    assert_grad_close("means2D", t["means2D"].grad.cpu().numpy(), rb["dmean2D"])
    assert_grad_close("means3D", t["means3D"].grad.cpu().numpy(), rb["dmeans3D"])
    assert_grad_close("opacities", t["opacities"].grad.cpu().numpy(), rb["dopacity"][:, None])
    if pb.D:
        assert_grad_close("language_feature_precomp", t["language_feature_precomp"].grad.cpu().numpy(), rb["dlang"])
