"""Fused densify-and-prune and opacity reset (langsplatv2_amd/densify.py,
csrc/densify.hip) against the reference's GaussianModel.densify_and_prune /
reset_opacity (scene/gaussian_model.py:303-306, 352-504).

CPU: `densify_and_prune_torch`, the reference's op sequence restated in torch,
equals tests/golden/ref_densify.npz (made by the reference's own methods:
tests/golden/make_ref_densify.py) bit for bit; argument checks; the C ABI's
codes for arguments rejected before any GPU use.

GPU: the fused path against `densify_and_prune_torch` run in float64 on the CPU
from the same fp32 inputs and noise.  The inputs (tests/densify_cases.py) keep
every row clear of every threshold (asserted: `assert_bands`), so the row
classes, counts and order must agree exactly; every copied value and moment
must be bit-identical; the two computed fields of a split child are bounded by
a forward-error analysis of the kernel's own operation sequence, with
u = 2^-24 (one fp32 rounding), multiply / add / subtract rounded correctly
(<= u relative) and sqrtf, division, expf, logf budgeted at one ulp (<= 2 u,
the accuracy the HIP math library documents for them):

  xyz'_c = ((R_c0 v_0 + R_c1 v_1) + R_c2 v_2) + xyz_c,  v_k = expf(s_k) z_k
    |q|^2 (4 squares, 3 adds of positives) 4 u; sqrtf halves it and adds 2 u: 4 u;
    q_i = r_i / |q| 6 u; a product of two components 13 u, and |q_a q_b| <= 1/2,
    y^2 + z^2 <= 1, so every entry of R has absolute error <= 29 u
    (1 - 2 (y^2 + z^2): 2 (13 u + u) + u; 2 (x y - r z): 2 (13 u + u));
    v_k 3 u relative (expf 2 u, product u); each product R_ck v_k
    (29 + 3 + 1) u |v_k| with |R_ck| <= 1; three additions 3 u (S + |xyz_c|),
    S = sum_k exp(s_k) |z_k|:
        |error| <= (36 S + 3 |xyz_c|) u                                  XYZ_C = (36, 3)
  s'_c = logf(expf(s_c) / 1.6f): expf 2 u, the constant 1.6f u, the division 2 u, so the
    argument of logf is off by 5 u relative = 5 u absolute in the result, plus logf's own
    ulp 2 u |s'_c|:
        |error| <= (5 + 2 |s'_c|) u                                      SCALE_C = (5, 2)
  reset: p = 1 / (1 + expf(-o)) 5 u (expf 2 u, add u, division 2 u), min with 0.01f keeps
    that; 1 - p <= 1.07 u relative (p <= 0.01); p / (1 - p) 5 + 1.07 + 2 <= 8.1 u; logf:
        |error| <= (8.1 + 2 |result|) u                                  RESET_C = (8.1, 2)
Each bound is multiplied by 1.001 for the second-order terms.  No figure here was
fitted to the kernel's output.  Measured on one MI355X: children at most 0.27 (xyz) and
0.72 (scaling) of their bounds, reset_opacity 0.44.

Known miss: test_torch_restatement_equals_reference_golden asks `torch.equal` on every
tensor against a file written on one CPU.  The copied fields, moments, row order and counts
are machine-independent; a split child's xyz and scaling go through torch's fp32 `exp` /
`log`, which the CPU math library evaluates differently on different processors (on the
machine that wrote the golden, fp32 exp differs from the correctly rounded value on 10 of
the 1,200 log-scales).  On the host of the MI355X used here both cases fail at the first
compared tensor (xyz) for that reason; on the machine that wrote the file they pass.  The
check is left as set.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from densify_cases import GROUPS, KNOBS, assert_bands, expected_classes, make_case
from langsplatv2_amd import _lib
from langsplatv2_amd.densify import (DensifyResult, densify_and_prune, densify_and_prune_torch, densify_tensors,
                                     reset_opacity)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_densify.npz")
U = 2.0 ** -24
SLACK = 1.001
XYZ_C, SCALE_C, RESET_C = (36.0, 3.0), (5.0, 2.0), (8.1, 2.0)
ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


# ------------------------------------------------------------------ helpers
def golden_case():
    z = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(z[k])   # noqa: E731
    case = {"params": {k: t(f"in_{k}") for k in GROUPS},
            "moments": {k: (t(f"in_{k}_exp_avg"), t(f"in_{k}_exp_avg_sq")) for k in GROUPS},
            "accum": t("in_accum"), "denom": t("in_denom"), "max_radii2D": t("in_max_radii2D"), "noise": t("noise")}
    return z, case


def run(fn, case, max_screen_size, device=None, dtype=None, knobs=KNOBS, **kw):
    mv = lambda t: t.to(device=device, dtype=dtype).contiguous()   # noqa: E731
    mom = {k: (None if m is None else tuple(mv(t) for t in m)) for k, m in case["moments"].items()}
    return fn({k: mv(v) for k, v in case["params"].items()}, mom, mv(case["accum"]), mv(case["denom"]),
              mv(case["max_radii2D"]), max_screen_size=max_screen_size, noise=mv(case["noise"]), **knobs, **kw)


def expected_map(case, max_screen_size, KNOBS=KNOBS):
    """(source row, kind) of every output row, classified in float64: the four stably compacted segments."""
    acc, den = case["accum"].double().reshape(-1), case["denom"].double().reshape(-1)
    g = acc / den
    g[g.isnan()] = 0.0
    s = case["params"]["scaling"].double()
    ms = torch.exp(s).max(dim=1).values
    sel = g >= KNOBS["max_grad"]
    small = ms <= KNOBS["percent_dense"] * KNOBS["extent"]
    faint = torch.sigmoid(case["params"]["opacity"].double()).reshape(-1) < KNOBS["min_opacity"]
    no = torch.zeros_like(faint)
    gone = faint | (ms > 0.1 * KNOBS["extent"] if max_screen_size else no)
    gone_child = faint | (ms / 1.6 > 0.1 * KNOBS["extent"] if max_screen_size else no)
    split, clone = sel & ~small, sel & small
    rows = torch.arange(len(g))
    segs = [rows[~split & ~gone], rows[clone & ~gone], rows[split & ~gone_child], rows[split & ~gone_child]]
    src = torch.cat(segs)
    kind = torch.cat([torch.full((len(r),), k) for k, r in enumerate(segs)])
    return src, kind, (int(clone.sum()), int(split.sum()))


def child_bounds(case, src, kind):
    """Per-element error bounds of xyz and scaling for the output rows (0 where the value is a copy)."""
    child = kind >= 2
    s = case["params"]["scaling"].double()[src]
    x = case["params"]["xyz"].double()[src]
    z = case["noise"].double()[src, (kind - 2).clamp(min=0)]
    S = (torch.exp(s) * z.abs()).sum(dim=1, keepdim=True)
    bx = (XYZ_C[0] * S + XYZ_C[1] * x.abs()) * U * SLACK
    bs = (SCALE_C[0] + SCALE_C[1] * (s - np.log(1.6)).abs()) * U * SLACK
    return bx * child[:, None], bs * child[:, None]


def check_fused(case, max_screen_size, got, ref64, label="", knobs=KNOBS):
    """got: densify_tensors' output (device); ref64: densify_and_prune_torch in float64 on the CPU."""
    gp, gm, gstats, gres = got
    rp, rm, _, rres = ref64
    src, kind, (n_clone, n_split) = expected_map(case, max_screen_size, knobs)
    n = case["params"]["xyz"].shape[0]
    assert rres == DensifyResult(n, n_clone, n_split, n + n_clone + n_split - len(src), len(src))
    assert gres == rres, (gres, rres)
    bx, bs = child_bounds(case, src, kind)
    worst = {}
    for k in GROUPS:
        g, r = gp[k].cpu(), rp[k]
        assert tuple(g.shape) == tuple(r.shape) and g.dtype == torch.float32
        if k in ("xyz", "scaling"):
            b = bx if k == "xyz" else bs
            err = (g.double() - r).abs()
            copied = (b == 0)
            assert torch.equal(g[copied], r.float()[copied]), k
            ratio = (err / b.clamp(min=1e-300))[~copied]
            worst[k] = float(ratio.max()) if ratio.numel() else 0.0
            assert bool((err <= b).all()), f"{k}: {worst[k]:.3f} x the bound"
        else:
            assert torch.equal(g, r.float()), k   # the float64 run only moved fp32 values: exact
        if rm[k] is None:
            assert gm[k] is None
        else:
            for a, b_ in zip(gm[k], rm[k]):
                assert torch.equal(a.cpu(), b_.float()), f"moment of {k}"
    for t, shape in zip(gstats, ((len(src), 1), (len(src), 1), (len(src),))):
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and not t.any()
    print(f"{label}: N {n} -> {len(src)} (clone {n_clone}, split {n_split}); children at "
          f"{worst.get('xyz', 0):.3f} (xyz) / {worst.get('scaling', 0):.3f} (scaling) of the bound")


def assert_mixed(case, max_screen_size):
    """The band condition, and at least N / 20 rows in every class."""
    assert_bands(case)
    n = case["params"]["xyz"].shape[0]
    c = expected_classes(case, max_screen_size)
    for k in ("clone", "split", "pruned_original", "pruned_child_parents"):
        assert c[k] * 20 >= n, (k, c)
    assert c["inf"] > 0 and c["nan"] > 0, c


# ---------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("tag,mss", [("none", None), ("s20", 20)])
def test_torch_restatement_equals_reference_golden(tag, mss):
    z, case = golden_case()
    assert_mixed(case, mss)
    P, M, stats, res = run(densify_and_prune_torch, case, mss)
    n_after = z[f"out_{tag}_xyz"].shape[0]
    for k in GROUPS:
        assert torch.equal(P[k], torch.from_numpy(z[f"out_{tag}_{k}"])), k
        assert torch.equal(M[k][0], torch.from_numpy(z[f"out_{tag}_{k}_exp_avg"])), k
        assert torch.equal(M[k][1], torch.from_numpy(z[f"out_{tag}_{k}_exp_avg_sq"])), k
        assert float(z[f"out_{tag}_{k}_step"]) == float(z[f"in_{k}_step"]) == 1.0
    for t, k in zip(stats, ("accum", "denom", "max_radii2D")):
        assert torch.equal(t, torch.from_numpy(z[f"out_{tag}_{k}"])) and not t.any()
    src, _, (n_clone, n_split) = expected_map(case, mss)
    assert n_split == int(z[f"out_{tag}_n_split"])
    assert res == DensifyResult(400, n_clone, n_split, 400 + n_clone + n_split - n_after, n_after)
    assert len(src) == n_after


def test_max_radii_has_no_effect_and_float64_agrees():
    """The reference zeroes max_radii2D before its final prune: any value gives the same result."""
    _, case = golden_case()
    a = run(densify_and_prune_torch, case, 20)
    b = run(densify_and_prune_torch, dict(case, max_radii2D=torch.full((400,), 1e6)), 20)
    c = run(densify_and_prune_torch, case, 20, dtype=torch.float64)
    assert a[3] == b[3] == c[3]
    for k in GROUPS:
        assert torch.equal(a[0][k], b[0][k])
        assert torch.equal(a[0]["f_rest"], c[0]["f_rest"].float())


def _state_and_opt(case, fused_adam, device="cpu", step=True):
    from langsplatv2_amd.train_loop import GaussianState
    n = case["params"]["xyz"].shape[0]
    gs = GaussianState(torch.zeros(n, 3), torch.zeros(n, case["params"]["f_rest"].shape[1] + 1, 3),
                       torch.full((n, 1), 0.5), torch.ones(n, 3), torch.ones(n, 4))
    for k, a in zip(GROUPS, ATTRS):
        setattr(gs, a, case["params"][k].clone().to(device).requires_grad_(True))
    gs.xyz_gradient_accum, gs.denom = case["accum"].clone().to(device), case["denom"].clone().to(device)
    gs.max_radii2D = case["max_radii2D"].clone().to(device)
    opt = gs.optimizer(fused=fused_adam)
    if step:
        gen = torch.Generator().manual_seed(3)
        for p in gs.params():
            p.grad = torch.randn(p.shape, generator=gen).to(device)
        opt.step()
        opt.zero_grad(set_to_none=True)
    return gs, opt


def test_reset_opacity_torch_equals_reference_golden():
    z, case = golden_case()
    gs, opt = _state_and_opt(case, fused_adam=False, step=False)
    # the golden's moments and step, as its optimiser held them before the reset
    for k, a in zip(GROUPS, ATTRS):
        opt.state[getattr(gs, a)] = {"step": torch.tensor(1.0), "exp_avg": case["moments"][k][0].clone(),
                                     "exp_avg_sq": case["moments"][k][1].clone()}
    reset_opacity(gs, opt, fused=False)
    st = opt.state[gs._opacity]
    assert opt.param_groups[3]["params"][0] is gs._opacity and gs._opacity.requires_grad and gs._opacity.is_leaf
    assert torch.equal(gs._opacity.detach(), torch.from_numpy(z["reset_opacity"]))
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == 1.0
    # the reference's own fp32 error is inside the bound the GPU test allows the kernel
    o = case["params"]["opacity"].double()
    p = torch.minimum(torch.sigmoid(o), torch.tensor(0.01, dtype=torch.float32).double())
    exact = torch.log(p / (1 - p))
    bound = (RESET_C[0] + RESET_C[1] * exact.abs()) * U * SLACK
    assert bool(((torch.from_numpy(z["reset_opacity"]).double() - exact).abs() <= bound).all())


def test_argument_checks():
    case = make_case(8, 0, coeffs=4)
    for fn in (densify_tensors, densify_and_prune_torch):
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="max_grad"):
                fn(case["params"], case["moments"], case["accum"], case["denom"], case["max_radii2D"],
                   max_grad=bad, min_opacity=0.005, extent=4.0, max_screen_size=None, noise=case["noise"])
    with pytest.raises(ValueError, match="scaling"):
        run(densify_tensors, dict(case, params=dict(case["params"], scaling=torch.zeros(8, 4))), None)
    with pytest.raises(ValueError, match="f_rest"):
        run(densify_tensors, dict(case, params=dict(case["params"], f_rest=torch.zeros(7, 3, 3))), None)
    with pytest.raises(ValueError, match="noise"):
        run(densify_tensors, dict(case, noise=torch.zeros(8, 3, 2)), None)
    with pytest.raises(ValueError, match="denom"):
        run(densify_tensors, dict(case, denom=torch.zeros(9, 1)), None)
    with pytest.raises(ValueError, match="exp_avg"):
        run(densify_tensors, dict(case, moments=dict(case["moments"], xyz=(torch.zeros(8, 3), torch.zeros(8, 4)))), None)
    with pytest.raises(ValueError, match="lacks"):
        densify_tensors({"xyz": case["params"]["xyz"]}, None, case["accum"], case["denom"], case["max_radii2D"],
                        max_screen_size=None, **KNOBS)
    # non-contiguous and non-fp32 inputs are refused by the fused path (the C ABI takes raw pointers)
    params = dict(case["params"], rotation=torch.zeros(4, 8).t())
    with pytest.raises(ValueError, match="contiguous"):
        densify_tensors(params, case["moments"], case["accum"], case["denom"], case["max_radii2D"],
                        max_screen_size=None, noise=case["noise"], **KNOBS)
    with pytest.raises(ValueError, match="float32"):
        run(densify_tensors, case, None, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        run(densify_tensors, case, None)
    gs, opt = _state_and_opt(case, fused_adam=False, step=False)
    with pytest.raises(RuntimeError, match="ROCm"):
        reset_opacity(gs, opt)
    opt.param_groups[0]["name"] = "positions"
    with pytest.raises(ValueError, match="group named"):
        densify_and_prune(gs, opt, max_screen_size=None, noise=case["noise"], **KNOBS)


def test_c_abi_codes_before_any_gpu_use():
    lib = _lib.load()
    OK, EINVAL, EUNSUPPORTED = 0, 1, 2
    counts = (ctypes.c_int64 * 6)(*([7] * 6))
    big = (1 << 28) + 1
    assert lib.lsr_densify_workspace_bytes(-1) == 0 and lib.lsr_densify_workspace_bytes(big) == 0
    assert lib.lsr_densify_workspace_bytes(1000) >= 1000 * 32
    plan = lambda n, mg=2e-4, cnt=counts, p=None: lib.lsr_densify_plan(   # noqa: E731
        n, p, p, p, p, mg, 0.04, 0.005, 0, 0.4, p, cnt, None)
    assert plan(-1) == EINVAL
    assert plan(10, mg=0.0) == EINVAL and plan(10, mg=-1.0) == EINVAL and plan(10, mg=float("nan")) == EINVAL
    assert plan(10, cnt=None) == EINVAL
    assert plan(big) == EUNSUPPORTED
    assert plan(10) == EINVAL                      # NULL tensors
    assert plan(0) == OK and list(counts) == [0] * 6   # no rows: no GPU work, counts cleared
    ptrs = (ctypes.c_void_p * 18)()
    apply = lambda n, n_out, ws=None, rest=9, s=ptrs, d=ptrs, z=None: lib.lsr_densify_apply(   # noqa: E731
        n, n_out, ws, rest, s, d, z, None)
    assert apply(-1, 1) == EINVAL and apply(1, -1) == EINVAL and apply(1, 1, rest=-3) == EINVAL
    assert apply(big, 1) == EUNSUPPORTED
    assert apply(0, 0) == OK and apply(5, 0) == OK
    assert apply(5, 5) == EINVAL                                   # NULL workspace
    assert apply(5, 5, ws=256, s=None) == EINVAL and apply(5, 5, ws=256, z=None) == EINVAL
    assert apply(5, 5, ws=256, z=256) == EINVAL                    # a parameter without destination
    assert lib.lsr_reset_opacity(-1, None, None, None, None) == EINVAL
    assert lib.lsr_reset_opacity(0, None, None, None, None) == OK
    assert lib.lsr_reset_opacity(4, None, None, None, None) == EINVAL
    assert lib.lsr_abi_version() == 12


def test_schedule_follows_the_reference_loop():
    from langsplatv2_amd.train_loop import DensifyConfig, densify_schedule
    cfg = DensifyConfig(extent=1.0)
    fired = {it: densify_schedule(cfg, it - 1, 1) for it in range(1, 15100)}
    for it, (d, size, reset) in fired.items():
        on = it < 15000 and it > 500 and it % 100 == 0          # train.py:248-255
        assert d == (it if on else None)
        assert size == (20 if on and it > 3000 else None)
        assert reset == (it < 15000 and it % 3000 == 0)          # train.py:257
    assert densify_schedule(DensifyConfig(extent=1.0, white_background=True), 499, 1) == (None, None, True)
    # a window of 8 iterations fires what any of its iterations fires, once
    assert densify_schedule(cfg, 596, 8) == (600, None, False)
    assert densify_schedule(cfg, 2996, 8) == (3000, None, True)
    assert densify_schedule(cfg, 3096, 8) == (3100, 20, False)


# ---------------------------------------------------------------- GPU tests
CASES = {
    "n300": dict(n=300, seed=1),
    "n300_deg1_no_moments": dict(n=300, seed=2, coeffs=4, moments=False),
    "two_scan_tiles_plus_37": dict(n=2 * 4096 + 37, seed=3),
    "one_row_split": dict(n=1, seed=4, pick=(3, 3, 4)),
    "one_row_clone": dict(n=1, seed=5, pick=(4, 0, 3)),
    "one_row_pruned": dict(n=1, seed=6, pick=(0, 2, 0)),
    "one_row_nan_kept": dict(n=1, seed=7, pick=(5, 1, 5)),
    "prune_all": dict(n=300, seed=8, kind="prune_all"),
    "none_selected": dict(n=300, seed=9, kind="none"),
}
MIXED = ("n300", "n300_deg1_no_moments", "two_scan_tiles_plus_37")


@pytest.mark.gpu
@pytest.mark.parametrize("mss", [None, 20], ids=["no_size_limit", "size_limit"])
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_fused_against_float64(gpu, name, mss):
    case = make_case(**CASES[name])
    assert_bands(case)
    if name in MIXED:
        assert_mixed(case, mss)
    ref64 = run(densify_and_prune_torch, case, mss, dtype=torch.float64)
    got = run(densify_tensors, case, mss, device=gpu)
    check_fused(case, mss, got, ref64, f"{name}/{mss}")
    n = case["params"]["xyz"].shape[0]
    if name == "prune_all":
        assert got[3].n_after == 0 and all(got[0][k].shape[0] == 0 for k in GROUPS)
    if name == "none_selected":
        assert got[3] == DensifyResult(n, 0, 0, 0, n)
        for k in GROUPS:   # the values are the inputs, the moments kept; the statistics still zeroed (check_fused)
            assert torch.equal(got[0][k].cpu(), case["params"][k])
            assert torch.equal(got[1][k][0].cpu(), case["moments"][k][0])
            assert torch.equal(got[1][k][1].cpu(), case["moments"][k][1])


@pytest.mark.gpu
def test_gpu_golden_inputs(gpu):
    """The reference's own output rows: copied fields bit for bit, children within the bounds."""
    z, case = golden_case()
    for tag, mss in (("none", None), ("s20", 20)):
        got = run(densify_tensors, case, mss, device=gpu)
        check_fused(case, mss, got, run(densify_and_prune_torch, case, mss, dtype=torch.float64), f"golden/{tag}")
        for k in ("f_dc", "f_rest", "opacity", "rotation"):
            assert torch.equal(got[0][k].cpu(), torch.from_numpy(z[f"out_{tag}_{k}"]))
        assert torch.equal(got[1]["xyz"][0].cpu(), torch.from_numpy(z[f"out_{tag}_xyz_exp_avg"]))


@pytest.mark.gpu
def test_gpu_deterministic_and_drawn_noise(gpu):
    case = make_case(2 * 4096 + 37, 11)
    a = run(densify_tensors, case, 20, device=gpu)
    b = run(densify_tensors, case, 20, device=gpu)
    assert a[3] == b[3]
    for k in GROUPS:
        assert torch.equal(a[0][k], b[0][k])
        assert torch.equal(a[1][k][0], b[1][k][0]) and torch.equal(a[1][k][1], b[1][k][1])
    # noise=None draws torch.randn((N, 2, 3), generator=...) on the device
    mv = lambda t: t.to(gpu)   # noqa: E731
    args = ({k: mv(v) for k, v in case["params"].items()}, {k: tuple(map(mv, m)) for k, m in case["moments"].items()},
            mv(case["accum"]), mv(case["denom"]), mv(case["max_radii2D"]))
    drawn = densify_tensors(*args, max_screen_size=20, generator=torch.Generator(device=gpu).manual_seed(5), **KNOBS)
    noise = torch.randn((case["noise"].shape[0], 2, 3), device=gpu, generator=torch.Generator(device=gpu).manual_seed(5))
    given = densify_tensors(*args, max_screen_size=20, noise=noise, **KNOBS)
    assert torch.equal(drawn[0]["xyz"], given[0]["xyz"]) and not torch.equal(drawn[0]["xyz"], a[0]["xyz"])


@pytest.mark.gpu
def test_gpu_reset_opacity(gpu):
    z, case = golden_case()
    gs, opt = _state_and_opt(case, fused_adam=True, device=gpu)
    before = gs._opacity.detach().clone()
    steps = {k: float(opt.state[getattr(gs, a)]["step"]) for k, a in zip(GROUPS, ATTRS)}
    others = {a: getattr(gs, a) for a in ATTRS if a != "_opacity"}
    reset_opacity(gs, opt)
    st = opt.state[gs._opacity]
    assert opt.param_groups[3]["params"][0] is gs._opacity and gs._opacity.is_leaf and gs._opacity.requires_grad
    assert all(getattr(gs, a) is t for a, t in others.items())
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert {k: float(opt.state[getattr(gs, a)]["step"]) for k, a in zip(GROUPS, ATTRS)} == steps
    p = torch.minimum(torch.sigmoid(before.cpu().double()), torch.tensor(0.01, dtype=torch.float32).double())
    exact = torch.log(p / (1 - p))
    err = (gs._opacity.detach().cpu().double() - exact).abs()
    bound = (RESET_C[0] + RESET_C[1] * exact.abs()) * U * SLACK
    print(f"reset_opacity: worst {float((err / bound).max()):.3f} of the bound")
    assert bool((err <= bound).all())
    # the golden's inputs: against the reference's fp32 values, whose own error the CPU test holds to the same bound
    gs, opt = _state_and_opt(case, fused_adam=True, device=gpu, step=False)
    reset_opacity(gs, opt)
    ref = torch.from_numpy(z["reset_opacity"]).double()
    b2 = 2 * (RESET_C[0] + RESET_C[1] * ref.abs()) * U * SLACK
    assert bool(((gs._opacity.detach().cpu().double() - ref).abs() <= b2).all())
    assert gs._opacity not in opt.state or not opt.state[gs._opacity]   # no state before the first step: none made


@pytest.mark.gpu
@pytest.mark.parametrize("fused_adam", [True, False], ids=["FusedAdam", "torch_Adam"])
def test_gpu_optimizer_rewiring(gpu, fused_adam):
    case = make_case(300, 21)
    gs, opt = _state_and_opt(case, fused_adam, device=gpu)
    stepped = dict(case, params={k: getattr(gs, a).detach().cpu() for k, a in zip(GROUPS, ATTRS)})
    assert_bands(stepped)   # one Adam step moved scaling by 0.005 and opacity by 0.05
    old_m = {k: tuple(opt.state[getattr(gs, a)][m].clone() for m in ("exp_avg", "exp_avg_sq"))
             for k, a in zip(GROUPS, ATTRS)}
    noise = case["noise"].to(gpu)
    res = densify_and_prune(gs, opt, max_screen_size=20, noise=noise, **KNOBS)
    src, kind, (n_clone, n_split) = expected_map(stepped, 20)
    assert res == DensifyResult(300, n_clone, n_split, 300 + n_clone + n_split - len(src), len(src))
    kept = src[kind == 0].to(gpu)
    assert 0 < len(kept) < res.n_after
    for g, (k, a) in zip(opt.param_groups, zip(GROUPS, ATTRS)):
        p = getattr(gs, a)
        assert g["name"] == k and g["params"][0] is p and p.is_leaf and p.requires_grad and p.grad is None
        assert p.shape[0] == res.n_after and len(opt.state) == 6
        st = opt.state[p]
        assert float(st["step"]) == 1.0
        for m, old in zip(("exp_avg", "exp_avg_sq"), old_m[k]):
            assert st[m].shape == p.shape
            assert torch.equal(st[m][: len(kept)], old[kept])      # the surviving rows keep their moments
            assert not st[m][len(kept):].any()                     # clones and children start from zero
    for t, shape in ((gs.xyz_gradient_accum, (res.n_after, 1)), (gs.denom, (res.n_after, 1)),
                     (gs.max_radii2D, (res.n_after,))):
        assert tuple(t.shape) == shape and not t.any()
    before = [p.detach().clone() for p in gs.params()]
    for p in gs.params():
        p.grad = torch.ones_like(p)
    opt.step()
    for p, b in zip(gs.params(), before):
        assert float(opt.state[p]["step"]) == 2.0 and torch.isfinite(p).all() and not torch.equal(p.detach(), b)
    # fused=False rewires the same way and gives the same rows
    gs2, opt2 = _state_and_opt(case, fused_adam, device=gpu)
    assert densify_and_prune(gs2, opt2, max_screen_size=20, noise=noise, fused=False, **KNOBS) == res
    assert torch.equal(gs2._features_rest, before[2]) and opt2.param_groups[2]["params"][0] is gs2._features_rest


@pytest.mark.gpu
def test_gpu_trainer_densifies(gpu, monkeypatch):
    from langsplatv2_amd import densify as D
    from langsplatv2_amd import scenes
    from langsplatv2_amd.train_loop import DensifyConfig, GaussianState, RGBTrainer, render_rgb
    cam = scenes.make_camera(64, 64, device=gpu)
    g = scenes.make_gaussians(1000, cam, seed=4, sh_degree=3)
    target = GaussianState(*(g[k].to(gpu) for k in ("means3D", "shs", "opacities", "scales", "rotations")))
    target.active_sh_degree = 3
    gt = render_rgb(cam, target, torch.zeros(3, device=gpu))["render"].detach().clamp(0, 1)
    start = scenes.make_gaussians(1000, cam, seed=5, sh_degree=3)
    gs = GaussianState(*(start[k].to(gpu) for k in ("means3D", "shs", "opacities", "scales", "rotations")))
    cfg = DensifyConfig(extent=1.0, densify_from_iter=0, densification_interval=2, densify_grad_threshold=1e-6,
                        min_opacity=0.1, seed=9)
    captured = []
    real = D.densify_and_prune

    def spy(gs_, opt_, *, generator, **kw):
        """Record the inputs and draw the noise the call would draw, then run it on exactly those."""
        n = gs_._xyz.shape[0]
        noise = torch.randn((n, 2, 3), dtype=torch.float32, device=gs_._xyz.device, generator=generator)
        groups = {gr["name"]: gr for gr in opt_.param_groups}
        rec = {"params": {k: getattr(gs_, a).detach().clone() for k, a in zip(GROUPS, ATTRS)},
               "moments": {k: tuple(opt_.state[groups[k]["params"][0]][m].clone() for m in ("exp_avg", "exp_avg_sq"))
                           for k in GROUPS},
               "accum": gs_.xyz_gradient_accum.clone(), "denom": gs_.denom.clone(),
               "max_radii2D": gs_.max_radii2D.clone(), "noise": noise, "kw": kw}
        res = real(gs_, opt_, noise=noise, **kw)
        rec["res"] = res
        rec["after"] = {k: getattr(gs_, a).detach().clone() for k, a in zip(GROUPS, ATTRS)}
        rec["after_moments"] = {k: tuple(opt_.state[getattr(gs_, a)][m].clone() for m in ("exp_avg", "exp_avg_sq"))
                                for k, a in zip(GROUPS, ATTRS)}
        captured.append(rec)
        return res

    monkeypatch.setattr(D, "densify_and_prune", spy)
    tr = RGBTrainer(gs, torch.zeros(3, device=gpu), fused_loss=True, densify=cfg)
    exchanges, sizes, losses = [tr.exchange], [1000], []
    for _ in range(4):
        losses.append(tr.step(cam, gt))
        exchanges.append(tr.exchange)
        sizes.append(gs._xyz.shape[0])
    assert all(np.isfinite(losses)) and tr.iteration == 4
    assert len(captured) == 2                                     # iterations 2 and 4
    first, second = captured
    assert sizes == [1000, 1000, first["res"].n_after, first["res"].n_after, second["res"].n_after]
    assert first["res"].n_before == 1000 and second["res"].n_before == first["res"].n_after
    assert first["res"].n_clone > 0 and first["res"].n_split > 0 and first["res"].n_pruned > 0
    assert first["res"].n_after != 1000 and tr.last_densify == second["res"]
    assert exchanges[2] is not exchanges[1] and exchanges[4] is not exchanges[3] and exchanges[1] is exchanges[0]
    assert tr.exchange._params[0] is gs._xyz and gs.max_radii2D.shape[0] == sizes[-1]
    assert first["kw"]["max_screen_size"] is None and first["kw"]["fused"] is True
    # the state right after the first densification against fused=False (the reference's torch sequence) from the
    # same inputs and noise: same rows, copied values bit for bit; children within the bounds of the float64 run
    kw = {k: v for k, v in first["kw"].items() if k != "fused"}
    mss = kw.pop("max_screen_size")
    knobs = dict(max_grad=kw["max_grad"], min_opacity=kw["min_opacity"], extent=kw["extent"],
                 percent_dense=kw["percent_dense"])
    assert knobs == dict(max_grad=1e-6, min_opacity=0.1, extent=1.0, percent_dense=0.01)
    tp, tm, _, tres = run(densify_and_prune_torch, first, mss, knobs=knobs)
    assert tres == first["res"]
    for k in ("f_dc", "f_rest", "opacity", "rotation"):
        assert torch.equal(first["after"][k], tp[k]), k
        for got_m, torch_m in zip(first["after_moments"][k], tm[k]):
            assert torch.equal(got_m, torch_m), k
    case = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in first.items() if k in ("accum", "denom", "noise")}
    case["max_radii2D"] = first["max_radii2D"].cpu()
    case["params"] = {k: v.cpu() for k, v in first["params"].items()}
    case["moments"] = {k: tuple(t.cpu() for t in m) for k, m in first["moments"].items()}
    n_after = first["res"].n_after
    stats = (torch.zeros(n_after, 1), torch.zeros(n_after, 1), torch.zeros(n_after))
    check_fused(case, mss, (first["after"], first["after_moments"], stats, first["res"]),
                run(densify_and_prune_torch, case, mss, dtype=torch.float64, knobs=knobs), "trainer", knobs)
