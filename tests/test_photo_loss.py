"""Fused L1 + D-SSIM photometric loss (csrc/photo_loss.hip,
langsplatv2_amd.photo_loss).

CPU: the float64 torch `train_loop.view_loss` reproduces the vectors produced
by the reference's own l1_loss / ssim (tests/golden/make_ref_photo_loss.py), the
C ABI's return codes, the Python argument checks.
GPU: `photometric_loss` (forward + autograd backward through the C ABI) against
the golden vectors and against float64 `view_loss` on seeded shapes; the loss
values within LOSS_ATOL, the gradient by max|grad - ref| / max|ref| <= GRAD_RTOL.

Tolerances (fp32 kernel vs float64 reference) are twice the worst error
measured over these cases on the MI355X (tools/photo_loss_err.py ->
profiles/photo_loss_err.json).  Measured there: l1, ssim and loss off by at
most 3.9e-8 (an ssim value, under one fp32 ulp of it; the combined loss
<= 1.9e-8 but for the ssim-only case's 3.3e-8), the gradient by at most 3.3e-5 on
the smooth cases (small D: the cancellation in e11 - mu1^2) and 4.9e-7 on
the noisy ones.  The formulation it replaces, fp32 `view_loss` run by torch
on the same GPU, is off the same float64 truth by up to 7.6e-8 (loss) and
5.1e-5 / 7.3e-7 (gradient, smooth / noisy) on the same cases.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from langsplatv2_amd import _lib
from langsplatv2_amd.train_loop import view_loss

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_photo_loss.npz")
GOLD_NAMES = ["noisy_3x11x17", "noisy_1x5x3", "smooth_3x33x65", "smooth_3x64x128", "smooth_2x3x24x40"]
# the last: 8,196 tiles of 64 x 16, past the 8,192-workgroup grid cap, so some workgroups take a second tile
RANDOM_SHAPES = [(3, 7, 9), (3, 16, 64), (3, 47, 130), (1, 12, 11), (3, 16 * 2731 + 1, 1)]
LAMBDA = 0.2
LOSS_ATOL = 7.7e-8   # 2 x 3.88e-8
GRAD_RTOL = 6.6e-5   # 2 x 3.32e-5


@functools.lru_cache(maxsize=None)
def _gold(name):
    z = np.load(GOLD)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}


def ref64(x, y, lam=LAMBDA):
    """float64 view_loss on the CPU: (l1, ssim, loss, dloss/dx)."""
    from langsplatv2_amd.train_loop import l1_loss, ssim
    xd = torch.from_numpy(np.asarray(x)).double().requires_grad_(True)
    yd = torch.from_numpy(np.asarray(y)).double()
    loss = view_loss(xd, yd, lam)
    loss.backward()
    with torch.no_grad():
        return l1_loss(xd, yd).item(), ssim(xd, yd).item(), loss.item(), xd.grad.numpy()


@functools.lru_cache(maxsize=None)
def random_case(shape):
    rng = np.random.default_rng(sum(shape) * 7 + shape[-1])
    y = rng.random(shape, dtype=np.float32)
    x = np.clip(y + 0.2 * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return (x, y) + ref64(x, y)


def grad_err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def gpu_loss(x, y, lam=LAMBDA, scale=1.0):
    """(l1, ssim, loss, dloss/dx) of the fused pair on cuda:0."""
    from langsplatv2_amd.photo_loss import l1_ssim
    dev = torch.device("cuda:0")
    xt = torch.from_numpy(np.asarray(x)).to(dev).requires_grad_(True)
    l1, s = l1_ssim(xt, torch.from_numpy(np.asarray(y)).to(dev))
    loss = (1.0 - lam) * l1 + lam * (1.0 - s)
    (loss * scale).backward()
    return l1.item(), s.item(), loss.item(), xt.grad.cpu().numpy()


def check(got, ref, what):
    for k, name in enumerate(("l1", "ssim", "loss")):
        err = abs(got[k] - float(ref[k]))
        print(f"{what}: {name} error {err:.3g}")
    g = grad_err(got[3], ref[3])
    print(f"{what}: gradient relative error {g:.3g}")
    for k, name in enumerate(("l1", "ssim", "loss")):
        assert abs(got[k] - float(ref[k])) <= LOSS_ATOL, (what, name)
    assert g <= GRAD_RTOL, f"{what}: gradient relative error {g:.3g}"


# ---------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("name", GOLD_NAMES)
def test_float64_view_loss_matches_reference_golden(name):
    z = _gold(name)
    l1, s, loss, grad = ref64(z["x"], z["y"])
    assert abs(l1 - float(z["l1"])) <= 1e-12 * abs(float(z["l1"]))
    assert abs(s - float(z["ssim"])) <= 1e-12 * abs(float(z["ssim"]))
    assert abs(loss - float(z["loss"])) <= 1e-12 * abs(float(z["loss"]))
    assert grad_err(grad, z["grad"]) <= 1e-12


def test_golden_has_the_exact_patch():
    z = _gold("smooth_3x33x65")
    assert np.array_equal(z["x"][:, :16, :21], z["y"][:, :16, :21]) and not np.array_equal(z["x"], z["y"])


def test_return_code_table():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P = ctypes.cast(buf, ctypes.c_void_p).value   # a stand-in pointer, never dereferenced
    OK_ALLOC = _lib.ALLOC_FN(lambda ctx, n, which: 0)   # returns NULL: LSR_ENOMEM once validation passed
    NOALLOC = _lib.ALLOC_FN()   # a NULL allocator
    EINVAL, EUNSUP, ENOMEM = 1, 2, 4
    fwd = lib.lsr_photo_loss_forward     # (image, gt, planes, H, W, out, partials, alloc, ctx, stream)
    for args, want in [
            ((P, P, 0, 4, 4, P, None, OK_ALLOC, None, None), EINVAL),
            ((P, P, 3, 0, 4, P, None, OK_ALLOC, None, None), EINVAL),
            ((P, P, 3, 4, -1, P, None, OK_ALLOC, None, None), EINVAL),
            ((None, P, 3, 4, 4, P, None, OK_ALLOC, None, None), EINVAL),
            ((P, None, 3, 4, 4, P, None, OK_ALLOC, None, None), EINVAL),
            ((P, P, 3, 4, 4, None, None, OK_ALLOC, None, None), EINVAL),
            ((P, P, 3, 4, 4, P, None, NOALLOC, None, None), EINVAL),
            ((P, P, 1, 1 << 16, 1 << 15, P, None, OK_ALLOC, None, None), EUNSUP),        # 2^31 elements
            ((P, P, 0x7fffffff, 0x7fffffff, 0x7fffffff, P, None, OK_ALLOC, None, None), EUNSUP),
            ((P, P, 1, 1 << 16, 1 << 15, None, None, OK_ALLOC, None, None), EINVAL),     # both: invalid wins
            ((None, P, 1, 1 << 16, 1 << 15, P, None, OK_ALLOC, None, None), EINVAL),     # both
            ((P, P, 1, 1 << 16, 1 << 15, P, None, NOALLOC, None, None), EINVAL),         # both
            ((P, P, 3, 4, 4, P, None, OK_ALLOC, None, None), ENOMEM),
            ((P, P, 1, (1 << 16) - 1, 1 << 15, P, P, OK_ALLOC, None, None), ENOMEM),     # 2^31 - 2^15: supported
    ]:
        assert fwd(*args) == want, (args, want)
    bwd = lib.lsr_photo_loss_backward    # (image, gt, planes, H, W, partials, grad_out, grad_image, stream)
    for args, want in [
            ((P, P, 0, 4, 4, P, P, P, None), EINVAL),
            ((P, P, 3, -2, 4, P, P, P, None), EINVAL),
            ((P, P, 3, 4, 0, P, P, P, None), EINVAL),
            ((None, P, 3, 4, 4, P, P, P, None), EINVAL),
            ((P, None, 3, 4, 4, P, P, P, None), EINVAL),
            ((P, P, 3, 4, 4, None, P, P, None), EINVAL),
            ((P, P, 3, 4, 4, P, None, P, None), EINVAL),
            ((P, P, 3, 4, 4, P, P, None, None), EINVAL),
            ((P, P, 2, 1 << 15, 1 << 15, P, P, P, None), EUNSUP),
            ((P, P, 2, 1 << 15, 1 << 15, None, P, P, None), EINVAL),   # both: invalid wins
            ((P, P, 2, 1 << 15, 1 << 15, P, P, None, None), EINVAL),   # both
    ]:
        assert bwd(*args) == want, (args, want)


def test_python_argument_checks():
    from langsplatv2_amd import photo_loss as PL
    a, b = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    for fn in (PL.photometric_loss, PL.l1_ssim, PL.ssim, PL.l1_loss):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            fn(a, b)
        with pytest.raises(ValueError):
            fn(a, torch.rand(3, 8, 9))
    with pytest.raises(ValueError):
        PL.ssim(a, b, window_size=7)
    with pytest.raises(ValueError):
        PL.ssim(a, b, size_average=False)
    import langsplatv2_amd
    assert langsplatv2_amd.photometric_loss is PL.photometric_loss and langsplatv2_amd.l1_ssim is PL.l1_ssim


# ---------------------------------------------------------------------- GPU ---
@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLD_NAMES)
def test_gpu_matches_reference_golden(gpu, name):
    z = _gold(name)
    check(gpu_loss(z["x"], z["y"]), (z["l1"], z["ssim"], z["loss"], z["grad"]), name)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_gpu_matches_float64_view_loss(gpu, shape):
    c = random_case(shape)
    check(gpu_loss(c[0], c[1]), c[2:], str(shape))


def _grad_of(fn, x, y):
    xt = x.clone().requires_grad_(True)
    out = fn(xt, y)
    out.backward()
    return out.detach(), xt.grad


@pytest.mark.gpu
def test_gpu_ssim_and_l1_alone(gpu):
    from langsplatv2_amd import photo_loss as PL
    x, y = (torch.from_numpy(a).to(gpu) for a in random_case((3, 47, 130))[:2])
    l1, g_l1 = _grad_of(PL.l1_loss, x, y)
    s, g_s = _grad_of(PL.ssim, x, y)
    # the g_l1-only and g_ssim-only parts of the pair's backward
    for k, (val, g) in enumerate(((l1, g_l1), (s, g_s))):
        xt = x.clone().requires_grad_(True)
        pair = PL.l1_ssim(xt, y)
        pair[k].backward()
        assert torch.equal(pair[k].detach(), val) and torch.equal(xt.grad, g)
    c = random_case((3, 47, 130))
    _, ref_s, _, ref_gs = ref64(c[0], c[1], lam=1.0)    # loss = 1 - ssim
    _, _, _, ref_gl = ref64(c[0], c[1], lam=0.0)        # loss = l1
    assert abs(s.item() - ref_s) <= LOSS_ATOL and abs(l1.item() - c[2]) <= LOSS_ATOL
    assert grad_err(-g_s.cpu().numpy(), ref_gs) <= GRAD_RTOL
    assert grad_err(g_l1.cpu().numpy(), ref_gl) <= GRAD_RTOL
    loss, g = _grad_of(lambda a, b: PL.photometric_loss(a, b, LAMBDA), x, y)
    combo = (1.0 - LAMBDA) * g_l1 - LAMBDA * g_s
    scale = g.abs().max().item()
    assert (combo - g).abs().max().item() <= 4 * np.finfo(np.float32).eps * scale   # one fma vs two roundings
    assert loss.item() == ((1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - s)).item()


@pytest.mark.gpu
def test_gpu_upstream_scale_and_gt_grad(gpu):
    from langsplatv2_amd.photo_loss import photometric_loss
    c = random_case((3, 16, 64))
    x = torch.from_numpy(c[0]).to(gpu).requires_grad_(True)
    y = torch.from_numpy(c[1]).to(gpu).requires_grad_(True)
    (3.5 * photometric_loss(x, y, LAMBDA)).backward()
    assert y.grad is None
    assert grad_err(x.grad.cpu().numpy(), 3.5 * c[5]) <= GRAD_RTOL
    x2 = torch.from_numpy(c[0]).to(gpu).requires_grad_(True)
    photometric_loss(x2, y.detach(), LAMBDA).backward()
    assert (x.grad - 3.5 * x2.grad).abs().max().item() <= 4 * np.finfo(np.float32).eps * x.grad.abs().max().item()


@pytest.mark.gpu
def test_gpu_no_grad_allocates_no_partials(gpu, monkeypatch):
    from langsplatv2_amd.photo_loss import photometric_loss
    lib = _lib.load()
    real, seen = lib.lsr_photo_loss_forward, []

    def spy(*args):
        seen.append(args[6])
        return real(*args)

    monkeypatch.setattr(lib, "lsr_photo_loss_forward", spy)
    c = random_case((3, 16, 64))
    x = torch.from_numpy(c[0]).to(gpu).requires_grad_(True)
    y = torch.from_numpy(c[1]).to(gpu)
    with torch.no_grad():
        a = photometric_loss(x, y, LAMBDA)
    b = photometric_loss(x.detach(), y, LAMBDA)
    d = photometric_loss(x, y, LAMBDA)
    assert seen[0] is None and seen[1] is None and seen[2] is not None
    assert not a.requires_grad and not b.requires_grad and d.requires_grad
    assert a.item() == b.item() == d.item()


@pytest.mark.gpu
def test_gpu_bit_reproducible(gpu):
    z = _gold("smooth_3x64x128")
    a, b = gpu_loss(z["x"], z["y"]), gpu_loss(z["x"], z["y"])
    assert a[:3] == b[:3] and np.array_equal(a[3], b[3])


@pytest.mark.gpu
def test_gpu_layouts_match_bitwise(gpu):
    from langsplatv2_amd.photo_loss import l1_ssim
    c = random_case((3, 47, 130))
    x = torch.from_numpy(c[0]).to(gpu)
    y = torch.from_numpy(c[1]).to(gpu)

    def run(xi, yi):
        xt = xi.clone().requires_grad_(True)
        l1, s = l1_ssim(xt, yi)
        (l1 - s).backward()
        return l1.item(), s.item(), xt.grad

    base = run(x, y)
    hwc = y.permute(1, 2, 0).contiguous().permute(2, 0, 1)   # an HWC image viewed as CHW
    assert not hwc.is_contiguous()
    got = run(x, hwc)
    assert got[:2] == base[:2] and torch.equal(got[2], base[2])
    # (B, C, H, W): the means run over all planes, so one batch of two equals the two halves' mean
    xb, yb = torch.stack((x, y)), torch.stack((y, x))
    gb = run(xb, yb)
    as_planes = run(xb.reshape(6, 47, 130), yb.reshape(6, 47, 130))
    assert gb[:2] == as_planes[:2] and torch.equal(gb[2].reshape(6, 47, 130), as_planes[2])
    assert gb[2].shape == xb.shape


@functools.lru_cache(maxsize=None)
def rendered_case():
    """One small view through the rasterizer: (image, gt) as numpy, 96 x 64, about 2K Gaussians."""
    from langsplatv2_amd.scenes import make_camera, make_gaussians
    from langsplatv2_amd.train_loop import GaussianState, render_rgb
    dev = torch.device("cuda:0")
    cam = make_camera(96, 64)
    g = make_gaussians(2000, cam, seed=3, sh_degree=3)
    gs = GaussianState(*(g[k].to(dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")))
    gs.active_sh_degree = 3
    img = render_rgb(cam, gs, torch.zeros(3, device=dev))["render"].detach()
    gen = torch.Generator().manual_seed(9)
    gt = (img.cpu() + 0.05 * torch.randn(3, 64, 96, generator=gen)).clamp(0, 1)
    return cam, g, img.cpu().numpy(), gt.numpy()


@pytest.mark.gpu
def test_gpu_through_the_rasterizer(gpu):
    from langsplatv2_amd.photo_loss import photometric_loss
    from langsplatv2_amd.train_loop import GaussianState, render_rgb
    cam, g, img_np, gt_np = rendered_case()
    gs = GaussianState(*(g[k].to(gpu) for k in ("means3D", "shs", "opacities", "scales", "rotations")))
    gs.active_sh_degree = 3
    image = render_rgb(cam, gs, torch.zeros(3, device=gpu))["render"]
    image.retain_grad()
    loss = photometric_loss(image, torch.from_numpy(gt_np).to(gpu), LAMBDA)
    loss.backward()
    assert np.array_equal(image.detach().cpu().numpy(), img_np)   # the forward render is bit-exact
    ref = ref64(img_np, gt_np)
    g_err = grad_err(image.grad.cpu().numpy(), ref[3])
    print(f"render: loss error {abs(loss.item() - ref[2]):.3g}, gradient {g_err:.3g}")
    assert abs(loss.item() - ref[2]) <= LOSS_ATOL
    assert g_err <= GRAD_RTOL
    assert gs._xyz.grad is not None and torch.isfinite(gs._xyz.grad).all() and gs._xyz.grad.abs().max() > 0


@pytest.mark.gpu
def test_gpu_trainer_fused_loss(gpu):
    from langsplatv2_amd.train_loop import GaussianState, RGBTrainer
    cam, g, _, gt_np = rendered_case()
    gt = torch.from_numpy(gt_np).to(gpu)
    losses = []
    for fused in (True, False):
        gs = GaussianState(*(g[k].to(gpu) for k in ("means3D", "shs", "opacities", "scales", "rotations")))
        tr = RGBTrainer(gs, torch.zeros(3, device=gpu), lambda_dssim=LAMBDA, fused_loss=fused)
        losses.append(tr.step(cam, gt))
    print(f"trainer first loss: fused {losses[0]!r}, torch {losses[1]!r}")
    assert abs(losses[0] - losses[1]) <= LOSS_ATOL
