"""Shared test helpers: build a seeded case, run it through the HIP path
(via the drop-in `diff_gaussian_rasterization` surface) and through the
oracle, and compare."""
from __future__ import annotations

import numpy as np
import torch

from langsplatv2_amd.scenes import make_camera, make_gaussians

# Backward tolerance (documented in DESIGN.md §Parity): GPU sums per-Gaussian
# gradients in fp32 (wave reduction + atomics, arrival order varies); the
# oracle sums the identical per-pair fp32 terms sequentially in fp64.
GRAD_RTOL = 1e-5     # relative to the tensor's max |value|
GRAD_ATOL = 1e-6
# Whole-frame backward at BASELINE cfg3 / D = 64 with N(0,1) upstream gradients
# on EVERY pixel (bench.py's workload, tests/test_fullsize.py): thousands of
# random-sign per-block rows cancel in each Gaussian's fp32 atomic sum, so the
# fp32-vs-fp64 summation error grows with the sum's length, and the preprocess
# backward's chain rule (conic -> cov2D -> cov3D -> scale / rotation) carries it
# on.  Measured (r05, gpurun_out/fullsize_grad_errors.json): at
# most 1.06e-5 x max|ref| (rotations), 6e-6 (scales), <= 1e-6 for the direct
# row sums (means2D, opacity, colour / SH, language).  The bound for these
# frames is 2x the worst measured.
GRAD_RTOL_FRAME = 2e-5
# Forward images: every forward kernel is bit-exact against the oracle (the
# deterministic expf_det in the blend).  A fast-exponential ML forward was built
# and measured in round 5 (hardware v_exp_f32 with the oracle's decisions kept by
# error-band re-decisions and an exact re-render of blocks with a termination
# test in the band): 5.5 % of the cfg3 blocks re-rendered and render_fwd went
# 0.310 -> 0.374 ms, so it is not in the product.  The helpers
# below keep the tolerance per case, 0 = bit-exact.
FWD_ATOL_FX = 0.0
FWD_ATOL = FWD_ATOL_FX


def fwd_atol(case) -> float:
    """The forward image tolerance of a case: FWD_ATOL_FX on the ML form
    (dense language channels > 8), else 0 (bit-exact)."""
    g = case["g"]
    lf = g.get("language_feature_precomp")
    D = 0 if (lf is None or case.get("quick")) else int(lf.shape[1])
    return FWD_ATOL_FX if D > 8 else 0.0


def assert_img(got, ref, atol, name=""):
    """One forward image against the oracle: bit-exact at atol 0, else max-abs <= atol."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if atol == 0:
        np.testing.assert_array_equal(got, ref, err_msg=name)
        return 0.0
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(initial=0.0))
    assert err <= atol, f"{name}: max|err|={err:.3e} > {atol:.1e}"
    return err


def make_case(N, W, H, seed=0, sh_degree=None, lang_dim=0, quick_k=0, yaw=0.0, cov_precomp=False, device="cpu",
              bg=(0.0, 0.0, 0.0), scale_modifier=1.0):
    cam = make_camera(W, H, yaw_deg=yaw)
    g = make_gaussians(N, cam, seed=seed, sh_degree=sh_degree, lang_dim=lang_dim, quick_k=quick_k)
    if cov_precomp:
        g["cov3D_precomp"] = cov3d_torch(g["scales"] * scale_modifier, g["rotations"]).float()
        del g["scales"], g["rotations"]
    return dict(cam=cam, g=g, bg=bg, scale_modifier=scale_modifier, quick=quick_k > 0)


def add_needles(case, frac=0.25, seed=0, sigma_px=(60.0, 600.0), angle_deg=(30.0, 60.0)):
    """Turn a fraction of the case's Gaussians into needle splats: one long axis
    whose projected sigma is log-uniform in `sigma_px` pixels, two tiny axes
    (the 0.3 px dilation then sets the short axis, so the 2D condition number
    is ~sigma^2 / 0.3 = 1e4 .. 1e6), rotated in the image plane by an angle
    uniform in `angle_deg` (either sign).  The camera looks along +z, so a
    rotation about z is an in-plane rotation.  The needles are the regime where
    det = ca cc - cb^2 of the fp32 conic loses most of its bits."""
    g = case["g"]
    assert "scales" in g, "needles need scales/rotations"
    N = g["means3D"].shape[0]
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(N, size=max(1, int(frac * N)), replace=False))
    cam = case["cam"]
    focal = cam["W"] / (2.0 * cam["tanfovx"])
    z = g["means3D"][idx, 2].numpy().astype(np.float64)
    z = np.where(z > 0.5, z, 5.0)
    sig = np.exp(rng.uniform(np.log(sigma_px[0]), np.log(sigma_px[1]), idx.size))
    s = np.stack([sig * z / focal, np.full(idx.size, 1e-5), np.full(idx.size, 1e-5)], 1)
    th = np.radians(rng.uniform(*angle_deg, idx.size)) * rng.choice([-1.0, 1.0], idx.size)
    q = np.stack([np.cos(th / 2), np.zeros_like(th), np.zeros_like(th), np.sin(th / 2)], 1)
    g["scales"][idx] = torch.from_numpy(s).float()
    g["rotations"][idx] = torch.from_numpy(q).float()
    return case


def trained_regime(case, factor, seed=0):
    """Turn a make_case frame into the regime of a trained scene: big, overlapping
    splats (every scale x `factor`), pixels that terminate early, saturated
    alphas, clamped SH colours and the projection's clamp quirk.  Works in camera
    space and rotates positions into the world by the view rotation, as
    make_gaussians does.  Rows 0..20 are overwritten:
      0..11   beyond the 1.3 tanfov clamp of t.x / t.z (even rows) and t.y / t.z
              (odd rows): |x/z| = 1.45 tanfov, z = 3 + k/2, scales 0.6..0.7,
              opacity 0.8 (test_oracle._grow's construction, on both axes);
      12      one giant, scales (5, 4, 3) (axis-aligned) at z = 4, opacity 0.3:
              it touches every tile of the frame;
      13..16  on the optical axis at view-space z = nextafter(0.2f, 1), 0.2f,
              nextafter(0.2f, 0), 0.25: around the near-plane cull (the positions
              are rotated into the world in float64 and rounded to fp32, so the
              kernel's fp32 view-space z is exactly these values only where the
              view rotation is the identity; in a yawed frame the rows lie within
              an ulp or two of the plane, on whichever side the rounding puts them);
      17..20  medium splats near the centre with opacity 0, 1/255,
              nextafter(1/255f, 1), 1: the alpha threshold and the 0.99 clamp.
    Of the other rows a seeded 15 % get opacity 0.999, and (SH input) a seeded
    25 % get 1.8 subtracted from their DC coefficients, so whole colours clamp
    at 0.  With cov3D_precomp the special rows' covariances are the diagonal
    ones of the same scale triples."""
    g, cam = case["g"], case["cam"]
    N = g["means3D"].shape[0]
    S = 21
    assert N > 2 * S
    rng = np.random.default_rng(seed)
    tx, ty = cam["tanfovx"], cam["tanfovy"]
    if "scales" in g:
        g["scales"] = g["scales"] * factor
    else:
        g["cov3D_precomp"] = g["cov3D_precomp"] * (factor * factor)
    pos = np.zeros((S, 3), np.float64)
    sc = np.zeros((S, 3), np.float32)
    op = np.zeros(S, np.float32)
    for k in range(12):
        z = 3.0 + 0.5 * k
        sgn = 1.0 if (k // 2) % 2 == 0 else -1.0
        off = 0.3 * (k % 3 - 1)
        pos[k] = (sgn * 1.45 * z * tx, off * z * ty, z) if k % 2 == 0 else (off * z * tx, sgn * 1.45 * z * ty, z)
        sc[k] = 0.6 + 0.1 * rng.random(3)
        op[k] = 0.8
    pos[12], sc[12], op[12] = (0.0, 0.0, 4.0), (5.0, 4.0, 3.0), 0.3
    near = np.float32(0.2)
    for j, z in enumerate((np.nextafter(near, np.float32(1)), near, np.nextafter(near, np.float32(0)),
                           np.float32(0.25))):
        pos[13 + j], sc[13 + j], op[13 + j] = (0.0, 0.0, float(z)), 0.002, 0.6
    thr = np.float32(1.0 / 255.0)
    for j, o in enumerate((np.float32(0.0), thr, np.nextafter(thr, np.float32(1)), np.float32(1.0))):
        pos[17 + j], sc[17 + j], op[17 + j] = ((j - 1.5) * 0.25, (1.5 - j) * 0.1, 5.0), (0.2, 0.15, 0.1), o
    wv = cam["viewmatrix"].cpu().t()[:3, :3].double()
    g["means3D"][:S] = (torch.from_numpy(pos) @ wv).float()
    g["opacities"][:S, 0] = torch.from_numpy(op)
    if "scales" in g:
        g["scales"][:S] = torch.from_numpy(sc)
        g["rotations"][12] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    else:
        s2 = (torch.from_numpy(sc).double() * case["scale_modifier"]) ** 2
        cov = torch.zeros(S, 6, dtype=torch.float64)
        cov[:, 0], cov[:, 3], cov[:, 5] = s2[:, 0], s2[:, 1], s2[:, 2]
        g["cov3D_precomp"][:S] = cov.float()
    rest = np.arange(S, N)
    opaque = np.sort(rng.choice(rest, size=int(round(0.15 * rest.size)), replace=False))
    g["opacities"][opaque] = 0.999
    if "shs" in g:
        dark = np.sort(rng.choice(rest, size=int(round(0.25 * rest.size)), replace=False))
        g["shs"][dark, 0] -= 1.8
    return case


def cov3d_torch(s, q):
    q = q.double()
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    L = R @ torch.diag_embed(s.double())
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def settings_for(case, device, layout=None):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    cam, g = case["cam"], case["g"]
    quick = case["quick"]
    return GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.tensor(case["bg"], dtype=torch.float32, device=device), scale_modifier=case["scale_modifier"],
        viewmatrix=cam["viewmatrix"].to(device), projmatrix=cam["projmatrix"].to(device),
        sh_degree=g.get("sh_degree", 0), campos=cam["campos"].to(device), prefiltered=False, debug=False,
        include_feature=("language_feature_precomp" in g) and not quick, quick_render=quick,
        language_feature_dim=g.get("quick_dim") if quick else None, language_feature_layout=layout)


def gpu_inputs(case, device, requires_grad=True):
    g = case["g"]
    t = {k: v.to(device) for k, v in g.items() if isinstance(v, torch.Tensor)}
    if requires_grad:
        for k in ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp",
                  "language_feature_precomp"):
            if k in t:
                t[k] = t[k].clone().requires_grad_(True)
    t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=requires_grad)
    return t


def run_gpu_forward(case, device, lang_layout=None, grad_request=0):
    """Forward through the library with workspace buffers decoded (lang_layout:
    the quick map's language_feature_layout: "chw" the reference's (Dq,H,W), None the
    default (pixel-major where the 12-code kernel applies), "hwc" pixel-major).
    grad_request (LSR_GWS_* bits): the forward of a call with a pending backward,
    as autograd runs it in training -- the render instantiation that also zeroes
    the backward's accumulators and, within the LSR_OPT_LISTS_MAX_MB budget,
    writes the per-block candidate lists; 0 is the inference forward.  The result
    says what that forward handed over: "has_grad_ws", "has_lists"."""
    from langsplatv2_amd import _lib, layout, rasterizer
    rs = settings_for(case, device, lang_layout)
    t = gpu_inputs(case, device, requires_grad=False)
    e = torch.empty(0, device=device)
    color, lang, radii, M, bufs, _, _, ws = rasterizer._run_forward(
        t["means3D"], t.get("shs", e), t.get("colors_precomp", e), t.get("language_feature_precomp", e),
        t.get("language_feature_weights_quick", e), t.get("language_feature_indices", e), t["opacities"],
        t.get("scales", e), t.get("rotations", e), t.get("cov3D_precomp", e), rs, grad_request)
    torch.cuda.synchronize()
    N = t["means3D"].shape[0]
    dec = layout.decode(bufs, N, rs.image_width, rs.image_height, M)
    out = {k: v.cpu().numpy() for k, v in dec.items()}
    out.update(color=color.cpu().numpy(), lang=lang.cpu().numpy(), radii=radii.cpu().numpy(), num_rendered=M,
               has_grad_ws=ws is not None, has_lists=bufs.get(_lib.LSR_BUF_LISTS) is not None)
    return out


def run_gpu_fwd_bwd(case, device, dout_color, dout_lang=None):
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = settings_for(case, device)
    t = gpu_inputs(case, device, requires_grad=True)
    r = GaussianRasterizer(raster_settings=rs)
    kw = {}
    for k in ("shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "language_feature_precomp",
              "language_feature_weights_quick", "language_feature_indices"):
        if k in t:
            kw[k] = t[k]
    color, lang, radii = r(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], **kw)
    outs, grads = [color], [torch.from_numpy(dout_color).to(device)]
    if dout_lang is not None and lang.numel() > 0 and lang.requires_grad:
        outs.append(lang)
        grads.append(torch.from_numpy(dout_lang).to(device))
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    res = dict(color=color.detach().cpu().numpy(), lang=lang.detach().cpu().numpy(), radii=radii.cpu().numpy())
    for k, v in t.items():
        if isinstance(v, torch.Tensor) and v.grad is not None:
            res["grad_" + k] = v.grad.cpu().numpy()
    return res


def oracle_problem(case):
    from oracle import oracle as O
    return O.Problem(case["cam"], case["g"], bg=case["bg"], scale_modifier=case["scale_modifier"],
                     quick=case["quick"])


def assert_image_close(got, ref, atol, decisions=True):
    """Forward images against the oracle.  `decisions`: n_contrib (the
    per-pixel termination / contribution decisions) bit-exact; final_T, colour
    and language within `atol` absolute (0: bit-exact).  Returns the max errors."""
    keys = ["color", "lang"] + (["final_T"] if decisions else [])
    if decisions:
        np.testing.assert_array_equal(got["n_contrib"], ref["n_contrib"].astype(np.int32))
    return {k: assert_img(got[k], ref[k], atol, k) for k in keys}


def grad_errors(got, ref):
    """Measured error of one gradient tensor: max-abs, max|ref|, their ratio,
    and whether the north_star's absolute 1e-5 holds."""
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    err = np.abs(got - ref)
    mref = float(np.abs(ref).max(initial=0.0))
    mabs = float(err.max(initial=0.0))
    big = np.abs(ref) >= 1e-3 * max(mref, 1e-30)
    return dict(max_abs=mabs, max_ref=mref, rel_to_max=mabs / mref if mref > 0 else 0.0,
                max_rel_elem_above_1em3max=float((err[big] / np.abs(ref[big])).max(initial=0.0)),
                p999_abs=float(np.quantile(err, 0.999)) if err.size else 0.0, abs_1e5=bool(mabs <= 1e-5), n=int(err.size))


def assert_grad_close(name, got, ref, rtol=GRAD_RTOL, atol=GRAD_ATOL):
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(1.0, float(np.abs(ref).max(initial=0.0)))
    err = float(np.abs(got - ref).max(initial=0.0))
    assert err <= atol + rtol * scale, f"{name}: max|err|={err:.3e} > {atol + rtol * scale:.3e} (max|ref|={scale:.3e})"
    return err, scale


def needle_contributing_tiles(out, W, H, band=4.0):
    """Per visible Gaussian of `out`: the tiles holding a pixel where the
    render's fp32 evaluation (splat_power, alpha = min(0.99, o exp(power)))
    gives alpha >= 1/255 and power <= 0.  Only pixels within `band` px of the
    long axis are evaluated (needles: the contributing band is < 2 px wide)."""
    xy, co, radii = out["xy"], out["conic_opacity"], out["radii"]
    gx = (W + 15) // 16
    res = {}
    for i in np.nonzero(radii > 0)[0]:
        x, y = xy[i]
        ca, cb, cc, o = (np.float32(v) for v in co[i])
        Q = np.array([[ca, cb], [cb, cc]], np.float64)
        w, V = np.linalg.eigh(Q)
        ax = V[:, 0]                      # long axis (smallest conic eigenvalue)
        half = 3.0 / np.sqrt(max(w[0], 1e-12))
        t = np.arange(-half, half + 1.0, 0.5)
        s = np.arange(-band, band + 0.5, 0.5)
        px = np.rint(x + t[:, None] * ax[0] + s[None, :] * ax[1]).astype(np.int64).ravel()
        py = np.rint(y + t[:, None] * ax[1] - s[None, :] * ax[0]).astype(np.int64).ravel()
        ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        pix = np.unique(py[ok] * W + px[ok])
        ys, xs = pix // W, pix % W
        dx = (np.float32(x) - xs.astype(np.float32)).astype(np.float32)
        dy = (np.float32(y) - ys.astype(np.float32)).astype(np.float32)
        p = np.float32(-0.5) * ((ca * dx) * dx + (cc * dy) * dy) - ((cb * dx) * dy)
        a = np.minimum(np.float32(0.99), o * np.exp(p.astype(np.float64)).astype(np.float32))
        m = (a >= np.float32(1 / 255.0)) & (p <= 0)
        res[int(i)] = set(((ys[m] // 16) * gx + xs[m] // 16).tolist())
    return res


def run_gpu_bwd_rows(case, device, dout_color, dout_lang=None, deterministic=True):
    """Forward + backward through the rasterizer's own autograd function bodies
    (rasterizer._run_forward / _RasterizeGaussians.backward), every input
    requiring grad, keeping the backward's gradient ROWS: the forward-prepared
    workspace the backward accumulates into (the deterministic backward's
    conversion pass writes every element of it) -- [0,1] dL/dmeans2D (NDC),
    [2..4] dL/dconic, [5] dL/dopacity, [6..8] dL/dcolour, lang columns per
    layout.  Returns {"rows": (N, VP), "VP": VP, "grad_<input>": ..., "has_lists":
    whether the forward handed the backward its per-block candidate lists}."""
    from types import SimpleNamespace

    from langsplatv2_amd import _lib, rasterizer
    rs = settings_for(case, device)
    t = gpu_inputs(case, device, requires_grad=False)
    e = torch.empty(0, device=device)
    lang_on = "language_feature_precomp" in t and not case["quick"]
    req = _lib.LSR_GWS_GEOM | (_lib.LSR_GWS_LANG if lang_on else 0)
    prev = _lib.set_deterministic(deterministic)
    try:
        color, lang, radii, M, bufs, saved, dims, ws = rasterizer._run_forward(
            t["means3D"], t.get("shs", e), t.get("colors_precomp", e), t.get("language_feature_precomp", e), e, e,
            t["opacities"], t.get("scales", e), t.get("rotations", e), t.get("cov3D_precomp", e), rs, req)
        assert ws is not None and ws[0] is not None
        has = lambda k: k in t  # noqa: E731
        need = (True, True, has("shs"), has("colors_precomp"), lang_on, False, False, True, has("scales"),
                has("rotations"), has("cov3D_precomp"), False)
        ctx = SimpleNamespace(raster_settings=rs, num_rendered=M, dims=dims, grad_ws=ws, needs_input_grad=need,
                              input_ids={}, saved_tensors=(*saved, radii, bufs[_lib.LSR_BUF_GEOM],
                                                           bufs[_lib.LSR_BUF_BINNING], bufs[_lib.LSR_BUF_IMAGE],
                                                           bufs.get(_lib.LSR_BUF_LISTS)))
        dl = torch.from_numpy(dout_lang).to(device) if (dout_lang is not None and lang_on) else None
        g = rasterizer._RasterizeGaussians.backward(ctx, torch.from_numpy(dout_color).to(device), dl, None)
        torch.cuda.synchronize()
    finally:
        _lib.set_deterministic(prev)
    N = t["means3D"].shape[0]
    VP = ws[1] // (4 * N)
    out = dict(rows=ws[0][:N * VP * 4].view(torch.float32).view(N, VP).cpu().numpy(), VP=VP,
               radii=radii.cpu().numpy(), num_rendered=M, has_lists=ctx.saved_tensors[-1] is not None)
    names = ("means3D", "means2D", "shs", "colors_precomp", "language_feature_precomp", None, None, "opacities",
             "scales", "rotations", "cov3D_precomp")
    for nm, v in zip(names, g):
        if nm is not None and v is not None:
            out["grad_" + nm] = v.cpu().numpy()
    return out
