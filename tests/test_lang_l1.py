"""The fused L1 (and normalised) language-feature loss, lsr_lang_l1_forward /
_backward behind language_l1_loss and language_feature_loss(fused_l1=True),
and language_gt_index's nearest-neighbour resize.

Checker: `ref_loss`, train.py:155-167 restated in float64 torch on the CPU and
differentiated by autograd (it must reproduce tests/golden/ref_lang_l1.npz,
which the reference's own l1_loss / cos_loss produced).  `l1_terms` is the
same loss and its gradients from the closed forms in DESIGN.md, in float64
numpy; it also reproduces the golden file, and it prices the ties.

Tolerances.  Loss: LOSS_ATOL = 2e-6 (tests/test_lang_loss_variants.py).
Gradients: GRAD_RTOL = 1e-5 of the pixel's largest |reference gradient| for
dL/dweight_map (the |f_p| = 0 pixels' is ~1e10 under --normalize) and of the
largest |entry| for dL/dcodebooks, plus a tie term.  L1's gradient jumps where
u_pd = g_pd; an fp32 kernel may take the other sign there, and no rounding
tolerance covers a jump.  Element (p, d) is a tie when, in float64,
|u_pd - g_pd| <= tau_pd = 8 K 2^-24 sum_k |C_kd w_pk| (8x the classical bound of
a 64-term fp32 dot product; under --normalize the band is 2 tau_pd / n_p).
Each tie adds the absolute change of every gradient entry when that element's
sigma flips by 2/(Df P).  The ties are few by assertion (at most 2e-4 of the
elements, at least 94 % of the pixels without one), so a wrong kernel fails on
the other pixels at the plain GRAD_RTOL."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import langsplatv2_amd
from langsplatv2_amd.lang_loss import language_feature_loss, language_gt_index, language_l1_loss

HERE = os.path.dirname(os.path.abspath(__file__))
LOSS_ATOL = 2e-6
GRAD_RTOL = 1e-5
K = 64
CONFIGS = {"l1": (False, False), "l1n": (True, False), "cl1n": (True, True)}   # name: (normalize, cos)
SHAPES = [(37, 53, 512, 23), (5, 70, 512, 3), (16, 64, 48, 7)]                 # H, W, Df, S: partial tiles
CASES = [(s, seed, False) for s in range(len(SHAPES)) for seed in range(3)] + [(0, 0, True)]


def ref_loss(wm, cb, seg, feat, normalize, cos, l1=True):
    """train.py:155-167 at layer 0 in float64 (scene/gaussian_model.py:533-543,
    scene/cameras.py:77-94, utils/loss_utils.py:18-25)."""
    D, H, W = wm.shape
    f = (cb[0].T @ wm.reshape(D, -1)).view(-1, H, W)
    if normalize:
        f = f / (f.norm(dim=0, keepdim=True) + 1e-10)
    sg = seg.long()
    mask = (sg != -1).unsqueeze(0)
    gt = feat[sg].permute(2, 0, 1)
    loss = torch.zeros((), dtype=torch.float64)
    if cos:
        loss = loss + 1 - F.cosine_similarity(f * mask, gt * mask, dim=0).mean()
    if l1:
        loss = loss + (f * mask - gt * mask).abs().mean()
    return loss


def ref_grads(wm, cb, seg, feat, normalize, cos):
    w64 = wm.double().requires_grad_(True)
    c64 = cb.double().requires_grad_(True)
    loss = ref_loss(w64, c64, seg, feat.double(), normalize, cos)
    loss.backward()
    return float(loss.detach()), w64.grad.numpy(), c64.grad.numpy()


def l1_terms(wm, cb, seg, feat, normalize, ties=False):
    """The L1 term from its closed forms (float64 numpy): loss, dL/dweight_map,
    dL/dcodebooks[0]; with `ties` also the tie mask (Df, P) and the tie terms
    of both gradients."""
    wm, cb, feat = (np.asarray(t, dtype=np.float64) for t in (wm, cb, feat))
    _, H, W = wm.shape
    P, Df, S = H * W, cb.shape[1], feat.shape[0]
    w = wm.reshape(K, P)
    f = cb.T @ w
    s = np.asarray(seg).reshape(-1)
    m = (s >= 0) & (s < S)
    g = np.where(m, feat[np.clip(s, 0, max(S - 1, 0))].T, 0.0)
    n = np.sqrt((f * f).sum(0))
    a = 1.0 / (n + 1e-10) if normalize else np.ones(P)
    diff = (a * f - g) * m
    c = 1.0 / (Df * P)
    sig = np.sign(diff) * c
    inv_n = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)      # torch's subgradient of the norm at 0
    dldf = a * sig - (a * a * inv_n * (f * sig).sum(0)) * f if normalize else sig
    out = [np.abs(diff).sum() * c, (cb @ dldf).reshape(K, H, W), w @ dldf.T]
    if not ties:
        return out
    tau = 8 * K * 2.0 ** -24 * (np.abs(cb).T @ np.abs(w))
    band = 2 * tau * inv_n if normalize else tau
    tie = m & (np.abs(diff) <= band)
    tol_w, tol_cb = np.zeros((K, P)), np.zeros((K, Df))
    for d, p in np.argwhere(tie):
        delta = np.zeros(Df)
        delta[d] = a[p] * 2 * c
        if normalize:
            delta -= a[p] ** 2 * inv_n[p] * f[d, p] * 2 * c * f[:, p]
        tol_w[:, p] += np.abs(cb @ delta)
        tol_cb += np.abs(np.outer(w[:, p], delta))
    return out + [tie, tol_w.reshape(K, H, W), tol_cb]


def _problem(H, W, Df, S, seed, unit=False):
    """test_lang_loss_variants._problem at K = 64 (sparse non-negative weight
    columns, Gaussian codebook and features), row 0 of the weight map zeroed
    (|f_p| = 0), optionally unit-norm feature rows (what CLIP's are)."""
    g = torch.Generator().manual_seed(seed)
    wm = torch.rand(K, H, W, generator=g) * (torch.rand(K, H, W, generator=g) < 0.2)
    cb = torch.randn(1, K, Df, generator=g)
    feat = torch.randn(S, Df, generator=g)
    seg = torch.randint(-1, S, (H, W), generator=g, dtype=torch.int32)
    wm[:, 0, :] = 0.0
    if unit:
        feat = feat / feat.norm(dim=1, keepdim=True)
    return wm, cb, seg, feat


@functools.lru_cache(maxsize=None)
def _case(shape, seed, unit):
    return _problem(*SHAPES[shape], seed, unit)


@functools.lru_cache(maxsize=None)
def _reference(shape, seed, unit, cfg):
    """(loss, dL/dweight_map, dL/dcodebooks, tie mask, tie terms) of one case, shared by the tests."""
    wm, cb, seg, feat = _case(shape, seed, unit)
    normalize, cos = CONFIGS[cfg]
    loss, gw, gcb = ref_grads(wm, cb, seg, feat, normalize, cos)
    _, _, _, tie, tol_w, tol_cb = l1_terms(wm.numpy(), cb[0].numpy(), seg.numpy(), feat.numpy(), normalize, ties=True)
    return loss, gw, gcb, tie, tol_w, tol_cb


def _gold():
    return dict(np.load(os.path.join(HERE, "golden", "ref_lang_l1.npz"), allow_pickle=False))


# --------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_restatement_matches_reference_losses(name, cfg):
    z = _gold()
    wm, cb, seg, feat = (torch.from_numpy(z[f"{name}_{k}"]) for k in ("weight_map", "codebooks", "seg", "features"))
    assert (seg == -1).any() and (wm.reshape(K, -1).abs().sum(0) == 0).any()
    normalize, cos = CONFIGS[cfg]
    loss, gw, gcb = ref_grads(wm, cb, seg, feat, normalize, cos)
    want_w, want_cb = z[f"{name}_{cfg}_grad_weight_map"], z[f"{name}_{cfg}_grad_codebooks"]
    assert abs(loss - float(z[f"{name}_{cfg}_loss"])) <= 1e-12
    np.testing.assert_allclose(gw, want_w, rtol=1e-9)
    np.testing.assert_allclose(gcb, want_cb, rtol=1e-9)
    if not cos:   # the closed forms the tie terms are priced with
        loss, gw, gcb = l1_terms(z[f"{name}_weight_map"], z[f"{name}_codebooks"][0], z[f"{name}_seg"],
                                 z[f"{name}_features"], normalize)
        assert abs(loss - float(z[f"{name}_{cfg}_loss"])) <= 1e-12
        np.testing.assert_allclose(gw, want_w, rtol=1e-9)
        np.testing.assert_allclose(gcb, want_cb[0], rtol=1e-9)


@pytest.mark.parametrize("shape,seed,unit", CASES)
@pytest.mark.parametrize("cfg", ["l1", "l1n"])
def test_ties_are_few(shape, seed, unit, cfg):
    """The tie term cannot hide a failure: few elements, and most pixels have none."""
    tie = _reference(shape, seed, unit, cfg)[3]
    print(f"tie elements {tie.mean():.3g}, pixels without a tie {1 - tie.any(0).mean():.4f}")
    assert tie.mean() <= 2e-4
    assert 1 - tie.any(0).mean() >= 0.94


def _resize_rule(src, H, W):
    """OpenCV resizeNN: x_src = min(floor(x * (1.0 / (W / Ws))), Ws - 1) in float64, rows alike."""
    Hs, Ws = src.shape
    ys = np.minimum(np.floor(np.arange(H) * (1.0 / (np.float64(H) / Hs))).astype(np.int64), Hs - 1)
    xs = np.minimum(np.floor(np.arange(W) * (1.0 / (np.float64(W) / Ws))).astype(np.int64), Ws - 1)
    return src[ys][:, xs]


@pytest.mark.parametrize("src,dst", [((1080, 1920), (540, 960)), ((738, 994), (369, 497)), ((369, 497), (738, 994)),
                                     ((1080, 1920), (728, 1295))])
def test_gt_index_resize(src, dst):
    rng = np.random.default_rng(src[0] + dst[1])
    maps = rng.integers(-1, 300, size=(4,) + src).astype(np.float32)   # <image>_s.npy holds floats
    for level in (0, 3):
        got = language_gt_index(maps, level, size=dst)
        assert got.dtype == torch.int32 and tuple(got.shape) == dst and got.is_contiguous()
        assert np.array_equal(got.numpy(), _resize_rule(maps[level].astype(np.int32), *dst))


def test_gt_index_without_size_is_unchanged():
    maps = np.random.default_rng(5).integers(-1, 40, size=(4, 23, 31)).astype(np.float32)
    want = torch.from_numpy(maps)[2].to(torch.int32)
    for kw in ({}, {"size": None}, {"size": (23, 31)}):
        got = language_gt_index(maps, 2, **kw)
        assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got, want)
    with pytest.raises(ValueError, match="feature_level"):
        language_gt_index(maps, 4, size=(5, 5))
    with pytest.raises(ValueError, match="size"):
        language_gt_index(maps, 0, size=(0, 5))


def test_l1_validation_on_cpu():
    wm, cb, seg, feat = _case(0, 0, False)
    assert langsplatv2_amd.language_l1_loss is language_l1_loss
    with pytest.raises(ValueError, match="language_l1_loss: weight_map"):
        language_l1_loss(wm[0], cb, seg, feat)
    with pytest.raises(ValueError, match="language_l1_loss: codebooks"):
        language_l1_loss(wm, cb[0, 0], seg, feat)
    with pytest.raises(ValueError, match="channels"):
        language_l1_loss(wm[:32], cb, seg, feat)
    with pytest.raises(ValueError, match="K must be 64"):
        language_l1_loss(wm, cb[:, :, :24], seg, feat[:, :24])
    with pytest.raises(ValueError, match="seg must be"):
        language_l1_loss(wm, cb, seg[:, :5], feat)
    with pytest.raises(ValueError, match="features must be"):
        language_l1_loss(wm, cb, seg, feat[:, :48])
    with pytest.raises(RuntimeError, match="language_l1_loss: weight_map .*no CPU path"):
        language_l1_loss(wm, cb, seg, feat)
    with pytest.raises(RuntimeError, match="no CPU path"):
        language_feature_loss(wm, cb, seg, feat, l1=True, fused_l1=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        language_feature_loss(wm, cb, seg, feat, l1=True, normalize=True, fused_l1=True)


# --------------------------------------------------------------------------- GPU

def _run(gpu, wm, cb, seg, feat, **flags):
    wg = wm.to(gpu).requires_grad_(True)
    cg = cb.to(gpu).requires_grad_(True)
    loss = language_feature_loss(wg, cg, seg.to(gpu), feat.to(gpu), **flags)
    loss.backward()
    return float(loss.detach()), wg.grad.double().cpu().numpy(), cg.grad.double().cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,seed,unit", CASES)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_fused_l1_matches_float64(gpu, shape, seed, unit, cfg):
    normalize, cos = CONFIGS[cfg]
    ref, ref_w, ref_cb, tie, tol_w, tol_cb = _reference(shape, seed, unit, cfg)
    assert tie.mean() <= 2e-4 and 1 - tie.any(0).mean() >= 0.94
    got, got_w, got_cb = _run(gpu, *_case(shape, seed, unit), normalize=normalize, cos=cos, l1=True, fused_l1=True)
    scale_w = np.maximum(np.abs(ref_w).max(0, keepdims=True), 1e-12)
    over_w = np.abs(got_w - ref_w) - (GRAD_RTOL * scale_w + tol_w)
    over_cb = np.abs(got_cb[0] - ref_cb[0]) - (GRAD_RTOL * np.abs(ref_cb).max() + tol_cb)
    print(f"loss {got:.9g} ref {ref:.9g} diff {abs(got - ref):.3g}; dL/dw worst rel "
          f"{(np.abs(got_w - ref_w) / scale_w).max():.3g} over {over_w.max():.3g}; dL/dcb worst rel "
          f"{np.abs(got_cb - ref_cb).max() / np.abs(ref_cb).max():.3g} over {over_cb.max():.3g}; ties {int(tie.sum())}")
    assert abs(got - ref) <= LOSS_ATOL, (got, ref)
    assert over_w.max() <= 0, f"dL/dweight_map exceeds its bound by {over_w.max():.3g}"
    assert over_cb.max() <= 0, f"dL/dcodebooks exceeds its bound by {over_cb.max():.3g}"
    assert float(np.abs(got_cb[1:]).max(initial=0.0)) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["l1", "l1n"])
def test_fused_l1_wide_features(gpu, cfg):
    """Df = 1040 (65 feature blocks): the backward's last sweep over the pixels has one block,
    for one wave of the four, and every sweep after the first adds into dL/dweight_map."""
    normalize, _ = CONFIGS[cfg]
    wm, cb, seg, feat = _problem(9, 21, 1040, 4, seed=7)
    ref, ref_w, ref_cb = ref_grads(wm, cb, seg, feat, normalize, False)
    _, _, _, tie, tol_w, tol_cb = l1_terms(wm.numpy(), cb[0].numpy(), seg.numpy(), feat.numpy(), normalize, ties=True)
    assert tie.mean() <= 2e-4 and 1 - tie.any(0).mean() >= 0.94
    got, got_w, got_cb = _run(gpu, wm, cb, seg, feat, normalize=normalize, cos=False, l1=True, fused_l1=True)
    assert abs(got - ref) <= LOSS_ATOL, (got, ref)
    scale_w = np.maximum(np.abs(ref_w).max(0, keepdims=True), 1e-12)
    assert (np.abs(got_w - ref_w) - (GRAD_RTOL * scale_w + tol_w)).max() <= 0
    assert (np.abs(got_cb[0] - ref_cb[0]) - (GRAD_RTOL * np.abs(ref_cb).max() + tol_cb)).max() <= 0


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [False, True])
def test_forward_is_deterministic(gpu, normalize):
    wm, cb, seg, feat = (t.to(gpu) for t in _case(0, 1, False))
    a = language_l1_loss(wm, cb, seg, feat, normalize=normalize)
    b = language_l1_loss(wm, cb, seg, feat, normalize=normalize)
    assert torch.equal(a, b) and bool(torch.isfinite(a))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_fused_matches_torch_path(gpu, cfg):
    normalize, cos = CONFIGS[cfg]
    wm, cb, seg, feat = (t.to(gpu) for t in _case(0, 2, False))
    fused = language_feature_loss(wm, cb, seg, feat, normalize=normalize, cos=cos, l1=True, fused_l1=True)
    plain = language_feature_loss(wm, cb, seg, feat, normalize=normalize, cos=cos, l1=True)
    print(f"fused {float(fused):.9g} torch {float(plain):.9g}")
    assert abs(float(fused) - float(plain)) <= 2 * LOSS_ATOL


@pytest.mark.gpu
def test_trainer_step_with_fused_l1(gpu):
    """LanguageTrainer(fused_l1=True) takes the step accumulate_language_views takes with the
    same flags (bounds of test_lang_loss_variants.test_trainer_step_with_l1_and_normalize)."""
    from langsplatv2_amd.train_loop import LanguageTrainer, accumulate_language_views
    from test_0_train_dp_lang import _scene
    flags = dict(normalize=True, cos=True, l1=True, fused_l1=True)
    cams, segs, feats, ls_a = _scene(gpu)
    _, _, _, ls_b = _scene(gpu)
    tr = LanguageTrainer(ls_a, torch.zeros(3, device=gpu), normalize=True, cos_loss=True, l1_loss=True, fused_l1=True)
    assert tr.loss_flags == flags
    la = tr.step(cams[0], segs[0], feats[0])
    ga = [g.detach().clone() for g in tr.last_grads]
    gb = []
    lb = accumulate_language_views(ls_b, ls_b.optimizer(), [cams[0]], [segs[0]], [feats[0]],
                                   torch.zeros(3, device=gpu), grads_out=gb, **flags)
    assert np.isfinite(la) and la == lb[0]
    for a, b in zip(ga, gb):
        assert float(b.abs().max()) > 0.0
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-12


@pytest.mark.gpu
def test_no_feature_wide_temporaries(gpu):
    """Peak allocation of forward + backward beyond the inputs grows by at most 1024 B per pixel:
    the outputs are 256 B/px (gradient map) + 8 B/px (stats) + 8 B/px of workspace, one fp32
    Df-wide row would be 2048 B/px."""
    def peak(H, W):
        g = torch.Generator().manual_seed(H)
        wm = (torch.rand(K, H, W, generator=g) * (torch.rand(K, H, W, generator=g) < 0.2)).to(gpu).requires_grad_(True)
        cb = torch.randn(1, K, 512, generator=g).to(gpu).requires_grad_(True)
        feat = torch.randn(9, 512, generator=g).to(gpu)
        seg = torch.randint(-1, 9, (H, W), generator=g, dtype=torch.int32).to(gpu)
        torch.cuda.synchronize(gpu)
        torch.cuda.reset_peak_memory_stats(gpu)
        base = torch.cuda.memory_allocated(gpu)
        language_feature_loss(wm, cb, seg, feat, normalize=True, cos=False, l1=True, fused_l1=True).backward()
        torch.cuda.synchronize(gpu)
        assert bool(torch.isfinite(wm.grad).all())
        return torch.cuda.max_memory_allocated(gpu) - base
    small, large = peak(128, 160), peak(256, 320)
    per_pixel = (large - small) / (256 * 320 - 128 * 160)
    print(f"peak beyond the inputs: {small} B at 128x160, {large} B at 256x320, {per_pixel:.1f} B per added pixel")
    assert per_pixel <= 1024
