"""GPU-vs-oracle parity in the regime of a trained scene: big, overlapping
splats (harness.trained_regime).  Every other default-suite case comes from
scenes.make_gaussians alone -- splats a few pixels wide, tile lists of at most
157, no early termination, nothing beyond the projection's clamp -- so these
frames are the first to reach, in the product's kernels,
  * the backward's walk from n_contrib of a pixel that terminated early,
  * a Gaussian spread over every 8x8 block of the frame,
  * the saturated alpha min(0.99, .) (upstream's straight-through gradient),
  * clamped SH colour channels (their gradient masked),
  * the 1.3 tanfov clamp quirk of the projection Jacobian.
tests/test_oracle.py pins the ORACLE to float64 autograd in this regime.

The forward is compared bit for bit; the backward is held to the derived
bounds of tests/test_deterministic.py (check_rows, check_chain): no tolerance
is introduced here."""
import functools

import numpy as np
import pytest
import torch

from harness import (GRAD_ATOL, GRAD_RTOL, assert_grad_close, gpu_inputs, grad_errors, make_case, oracle_problem,
                     run_gpu_bwd_rows, run_gpu_fwd_bwd, settings_for, trained_regime)
from test_deterministic import U, _check, _quant, _scales, _upstream, check_chain, check_rows, record
from test_gpu_parity import _fwd_compare

FRAMES = {
    # name: (make_case kwargs, factor)
    # factor 9: at 8 this frame's terminated share is 2.0 %, below the regime test's 3 % floor
    "sh3_lang16_bg": (dict(N=1500, W=160, H=112, sh_degree=3, lang_dim=16, seed=51, bg=(0.3, 0.6, 1.0)), 9),
    "sh2_lang32_yaw_ragged": (dict(N=3000, W=97, H=61, sh_degree=2, lang_dim=32, yaw=15.0, seed=52), 10),
    "rgb_lang3_cov": (dict(N=2500, W=128, H=80, lang_dim=3, cov_precomp=True, seed=53), 8),
    "sh1_lang64_scalemod": (dict(N=6000, W=64, H=48, sh_degree=1, lang_dim=64, scale_modifier=1.3, seed=54), 6),
    "rgb_nolang": (dict(N=2000, W=100, H=70, seed=55), 8),
    "sh3_lang24": (dict(N=2000, W=120, H=72, sh_degree=3, lang_dim=24, seed=56), 8),
    "quick192": (dict(N=2500, W=96, H=64, quick_k=4, seed=57), 8),
}
DENSE = [n for n in FRAMES if n != "quick192"]
VARIANTS = ["sh3_lang16_bg", "sh1_lang64_scalemod"]


def make_frame(name):
    kw, factor = FRAMES[name]
    return trained_regime(make_case(**kw), factor, seed=kw["seed"])


@functools.lru_cache(maxsize=None)
def _frame(name):
    """One frame, its oracle problem, forward and upstream gradients: computed
    once, shared by every test of the frame and never written to."""
    from oracle import oracle as O
    case = make_frame(name)
    pb = oracle_problem(case)
    ref = O.forward(pb)
    dcol, dlang = _upstream(pb.H, pb.W, pb.D)
    return case, pb, ref, dcol, dlang


@functools.lru_cache(maxsize=None)
def _frame_backward(name):
    """The oracle's backward of _frame(name) with its upstream gradients: once per frame."""
    from oracle import oracle as O
    case, pb, ref, dcol, dlang = _frame(name)
    return O.backward(pb, ref, dcol, dlang, nthreads=2)


def regime_figures(pb, ref):
    """The figures that make a frame 'trained regime', from the oracle's outputs alone."""
    counts = (ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0].astype(np.int64))
    ty, tx = np.divmod(np.arange(pb.H * pb.W).reshape(pb.H, pb.W), pb.W)
    per_pixel = counts[(ty // 16) * pb.gx + tx // 16]
    term = (ref["n_contrib"].astype(np.int64) < per_pixel) & (ref["final_T"] < 1e-3)
    vis = ref["radii"] > 0
    return dict(terminated=float(term.mean()), clamped=float(ref["clamped"][vis].mean()) if pb.shs is not None else 0.0,
                longest_list=int(counts.max()), largest_radius=int(ref["radii"].max()),
                most_tiles=int(ref["tiles_touched"].max()), tiles=pb.gx * pb.gy)


@pytest.mark.parametrize("name", list(FRAMES))
def test_frames_are_in_the_trained_regime(oracle_lib, name):
    """CPU only: the frames are what they claim, on the oracle's outputs."""
    case, pb, ref, dcol, dlang = _frame(name)
    fig = regime_figures(pb, ref)
    print(name, fig)
    assert fig["most_tiles"] == fig["tiles"]                  # the giant touches every tile
    assert ref["tiles_touched"][12] == fig["tiles"]
    assert fig["largest_radius"] >= 250
    V = case["cam"]["viewmatrix"].double().numpy()
    pv = case["g"]["means3D"].double().numpy() @ V[:3, :3] + V[3, :3]
    assert (ref["radii"][:12] > 0).all() and (ref["tiles_touched"][:12] > 0).all()   # visible, and reach the image
    ax = np.arange(12) % 2
    tan = np.where(ax == 0, case["cam"]["tanfovx"], case["cam"]["tanfovy"])
    assert (np.abs(pv[np.arange(12), ax] / pv[:12, 2]) > 1.3 * tan).all()
    near = ref["radii"][13:17] > 0
    assert near.any() and not near.all()
    for k, v in _frame_backward(name).items():
        if isinstance(v, np.ndarray):
            assert np.isfinite(v).all(), k
    assert fig["terminated"] >= 0.03
    if pb.shs is not None:
        assert fig["clamped"] >= 0.10


# ---------------------------------------------------------------- GPU forward

def _grad_request(case):
    """The LSR_GWS_* bits autograd asks the forward for when every input of the frame requires grad."""
    from langsplatv2_amd import _lib
    dense_lang = "language_feature_precomp" in case["g"] and not case["quick"]
    return _lib.LSR_GWS_GEOM | (_lib.LSR_GWS_LANG if dense_lang else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FRAMES))
def test_forward_bit_exact(gpu, oracle_lib, name):
    """The inference forward (no backward pending): geometry records, binning and
    images bit for bit (test_gpu_parity._fwd_compare)."""
    _fwd_compare(_frame(name)[0], gpu, oracle_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("lists", ["lists", "nolists"])
@pytest.mark.parametrize("name", DENSE)
def test_training_forward_bit_exact(gpu, oracle_lib, name, lists):
    """The forward of a call with a pending backward, as training runs it: the
    render instantiation that zeroes the backward's accumulators beside its own
    work and ("lists") writes each 8x8 block's candidate list, or
    (LSR_OPT_LISTS_MAX_MB = 0, "nolists") does not.  The same comparison, every
    output bit for bit.  (The quick forward takes no such request: the library
    prepares no dense backward for it, so the quick frame has the test above only.)"""
    from langsplatv2_amd import _lib
    case = _frame(name)[0]
    prev = _lib.set_lists_max_mb(0) if lists == "nolists" else None
    try:
        ref, got = _fwd_compare(case, gpu, oracle_lib, grad_request=_grad_request(case))
    finally:
        if prev is not None:
            _lib.set_lists_max_mb(prev)
    assert got["has_grad_ws"]                          # the accumulator-zeroing render ran
    assert got["has_lists"] == (lists == "lists")


# --------------------------------------------------------------- GPU backward

def _rel_to_max(got, rb):
    """For information: each returned gradient's max |err| / max |ref|, the
    measure GRAD_RTOL is stated in."""
    pairs = dict(means3D="dmeans3D", shs="dsh", colors_precomp="dcolor", scales="dscales", rotations="drot",
                 cov3D_precomp="dcov3D", language_feature_precomp="dlang", means2D="dmean2D")
    out = {}
    for k, r in pairs.items():
        if "grad_" + k in got and rb.get(r) is not None:
            out[k] = grad_errors(got["grad_" + k], rb[r])["rel_to_max"]
    out["opacities"] = grad_errors(got["grad_opacities"], rb["dopacity"])["rel_to_max"]
    return out


def _rows_and_chain(name, got, oracle_lib, deterministic, tag):
    case, _, _, dcol, dlang = _frame(name)
    pb, ref, r1 = check_rows(case, got, oracle_lib, dcol, dlang, deterministic=deterministic)
    r2 = check_chain(pb, ref, got, oracle_lib)
    res = {"rows": r1, "chain": r2, "rel_to_max_ref": _rel_to_max(got, _frame_backward(name))}
    print(tag, res)
    record(tag, res)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", DENSE)
def test_deterministic_backward(gpu, oracle_lib, name):
    """The fixed-point backward: two runs the same bits, render rows and chain
    rule within the derived bounds."""
    case, pb, ref, dcol, dlang = _frame(name)
    a = run_gpu_bwd_rows(case, gpu, dcol, dlang, deterministic=True)
    b = run_gpu_bwd_rows(case, gpu, dcol, dlang, deterministic=True)
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["has_lists"]
    assert float(np.abs(a["rows"]).max()) > 1e-3
    _rows_and_chain(name, a, oracle_lib, True, "trained_" + name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DENSE)
def test_default_backward(gpu, oracle_lib, name):
    """The float-atomic backward within the same analysis (any-order summation term)."""
    case, pb, ref, dcol, dlang = _frame(name)
    got = run_gpu_bwd_rows(case, gpu, dcol, dlang, deterministic=False)
    assert got["has_lists"]
    _rows_and_chain(name, got, oracle_lib, False, "trained_default_" + name)


@pytest.mark.gpu
@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "default"])
@pytest.mark.parametrize("name", VARIANTS)
def test_restaging_backward(gpu, oracle_lib, name, deterministic):
    """No per-block candidate lists from the forward: the backward re-stages its
    candidates from the tile lists (hundreds long here, with terminated pixels)."""
    from langsplatv2_amd import _lib
    case, pb, ref, dcol, dlang = _frame(name)
    prev = _lib.set_lists_max_mb(0)
    try:
        got = run_gpu_bwd_rows(case, gpu, dcol, dlang, deterministic=deterministic)
    finally:
        _lib.set_lists_max_mb(prev)
    assert not got["has_lists"]          # saved_tensors[-1] is None: the backward re-staged
    _rows_and_chain(name, got, oracle_lib, deterministic,
                    "trained_restage_" + ("" if deterministic else "default_") + name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
def test_language_only_backward(gpu, oracle_lib, name):
    """Only the language input requires grad (the language-only kernels):
    deterministic within bound + fixed-point term and bit-reproducible, default
    within bound + any-order term; as test_deterministic_language_only_backward."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from langsplatv2_amd import _lib
    case, pb, ref, dcol, dlang = _frame(name)
    t = gpu_inputs(case, gpu, requires_grad=False)
    lang = t["language_feature_precomp"].clone().requires_grad_(True)
    r = GaussianRasterizer(raster_settings=settings_for(case, gpu))

    def run(det):
        with _lib.deterministic(det):
            _, L, _ = r(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t["shs"],
                        scales=t["scales"], rotations=t["rotations"], language_feature_precomp=lang)
            (g,) = torch.autograd.grad(L, lang, torch.from_numpy(dlang).to(gpu))
        return g.cpu().numpy()
    g1, g2, gf = run(True), run(True), run(False)
    np.testing.assert_array_equal(g1, g2)
    rb = _frame_backward(name)
    bd = oracle_lib.backward_bound(pb, ref, dcol, dlang, with_mag=True)
    Dm, Am, WH = _scales(pb, ref, dcol, dlang)
    tol = bd["dlang"] + _quant(ref["radii"], 0, Dm, Am, WH)[:, None]
    res = {"deterministic": _check("language (deterministic)", g1, rb["dlang"], tol)}
    tol_f = bd["dlang"] + U * bd["nblocks"].astype(np.float64)[:, None] * bd["mag"]["dlang"]
    res["default"] = _check("language (default)", gf, rb["dlang"], tol_f)
    res["rel_to_max_ref"] = {"deterministic": grad_errors(g1, rb["dlang"])["rel_to_max"],
                             "default": grad_errors(gf, rb["dlang"])["rel_to_max"]}
    print(name, res)
    record("trained_langonly_" + name, res)


@pytest.mark.gpu
def test_quick_frame_backward(gpu, oracle_lib):
    """The quick frame's backward (RGB gradients; the quick map takes no upstream
    gradient here), as test_gpu_parity.test_backward_vs_oracle[quick192] asserts
    it: assert_grad_close against the oracle at the harness's standing
    GRAD_RTOL / GRAD_ATOL, now with tile lists of up to 225 and 24 % of the
    pixels terminated early.  That first criterion holds (the forward bit-exact),
    so the derived-bound fallback was not needed: measured max |err| / tolerance
    is 0.21 for scales, 0.08-0.09 rotations, 0.05 means2D, 0.04 means3D and
    colours, 0.03 opacities (float atomics: the figures move a little run to run)."""
    case, pb, ref, _, _ = _frame("quick192")
    H, W = pb.H, pb.W
    dcol = np.random.default_rng(1).standard_normal((3, H, W)).astype(np.float32)
    rb = oracle_lib.backward(pb, ref, dcol, None)
    got = run_gpu_fwd_bwd(case, gpu, dcol, None)
    np.testing.assert_array_equal(got["color"], ref["color"])
    np.testing.assert_array_equal(got["lang"], ref["lang"])
    pairs = [("means2D", rb["dmean2D"]), ("opacities", rb["dopacity"][:, None]), ("means3D", rb["dmeans3D"]),
             ("colors_precomp", rb["dcolor"]), ("scales", rb["dscales"]), ("rotations", rb["drot"])]
    fig = {}
    for k, r in pairs:
        e = grad_errors(got["grad_" + k], r)
        fig[k] = dict(max_abs=e["max_abs"], max_ref=e["max_ref"],
                      over_tol=e["max_abs"] / (GRAD_ATOL + GRAD_RTOL * max(1.0, e["max_ref"])))
    print("quick192", fig)
    record("trained_quick192", fig)
    for k, r in pairs:
        assert_grad_close(k, got["grad_" + k], r)
