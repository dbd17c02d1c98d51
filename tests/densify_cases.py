"""Inputs of the densification tests (tests/test_densify.py) and of the golden
generator (tests/golden/make_ref_densify.py).

Every quantity a threshold looks at comes from a small discrete set, so no row
lies near a threshold and a classification cannot flip on a rounding error:

  g = accum / denom   vs max_grad = 2e-4        {5e-5, 1e-4 | 4e-4, 1e-3, inf (x / 0)}, and 0 / 0 -> NaN -> 0
  ms = max exp(scaling) vs T = 0.01 * 4 = 0.04  {0.01, 0.02 | 0.1, 0.2, 0.5, 0.8}
  ms, ms / 1.6        vs 0.1 * 4 = 0.4          0.5 -> child 0.3125, 0.8 -> child 0.5
  opacity logit       vs logit(0.005) = -5.293  {-6, -5.5 | -5, -2, 0, 3}

`assert_bands` checks that on the tensors themselves (also after an optimiser
step moved them), `expected_classes` counts the rows of each class in float64.
"""
import math

import numpy as np
import torch

KNOBS = dict(max_grad=0.0002, min_opacity=0.005, extent=4.0, percent_dense=0.01)
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
G_CHOICES = (5e-5, 1e-4, 4e-4, 1e-3, "inf", "nan")
S_CHOICES = (0.01, 0.02, 0.1, 0.2, 0.5, 0.8)
O_CHOICES = (-6.0, -5.5, -5.0, -2.0, 0.0, 3.0)


def make_case(n: int, seed: int, coeffs: int = 16, kind: str = "mixed", pick=None, moments: bool = True) -> dict:
    """kind: "mixed" (uniform over the choices), "prune_all" (every opacity below the threshold), "none"
    (no gradient reaches max_grad, nothing is faint or big); pick = (g, s, o) choice indices forces every row."""
    rng = np.random.default_rng(seed)
    gi, si, oi = (rng.integers(0, 6, n) for _ in range(3))
    if kind == "prune_all":
        oi = rng.integers(0, 2, n)
    elif kind == "none":
        gi, si, oi = rng.integers(0, 2, n), rng.integers(0, 4, n), rng.integers(2, 6, n)
    if pick is not None:
        gi, si, oi = (np.full(n, p) for p in pick)
    denom = rng.choice([1.0, 2.0, 5.0], n).astype(np.float32)
    accum = np.zeros(n, np.float32)
    for i in range(n):
        c = G_CHOICES[gi[i]]
        if c == "inf":
            denom[i], accum[i] = 0.0, 0.3
        elif c == "nan":
            denom[i], accum[i] = 0.0, 0.0
        else:
            accum[i] = np.float32(c) * denom[i]
    ms = np.array([S_CHOICES[k] for k in si], np.float64)
    scal = np.log(ms)[:, None] + np.log(rng.uniform(0.3, 0.9, (n, 3)))
    scal[np.arange(n), rng.integers(0, 3, n)] = np.log(ms)
    # values the copy must move bit for bit: few distinct ones, so the golden file compresses
    lattice = lambda shape: rng.integers(-32, 33, shape).astype(np.float32) / 64.0   # noqa: E731
    params = {"xyz": rng.standard_normal((n, 3)).astype(np.float32) * 2,
              "f_dc": lattice((n, 1, 3)), "f_rest": lattice((n, coeffs - 1, 3)),
              "opacity": np.array([O_CHOICES[k] for k in oi], np.float32).reshape(n, 1),
              "scaling": scal.astype(np.float32),
              "rotation": (rng.standard_normal((n, 4)) * rng.choice([0.5, 1.0, 3.0], (n, 1))).astype(np.float32)}
    case = {"params": {k: torch.from_numpy(v) for k, v in params.items()},
            "accum": torch.from_numpy(accum).reshape(n, 1), "denom": torch.from_numpy(denom).reshape(n, 1),
            "max_radii2D": torch.from_numpy(rng.choice([0.0, 5.0, 50.0], n).astype(np.float32)),
            "noise": torch.from_numpy(rng.standard_normal((n, 2, 3)).astype(np.float32))}
    case["moments"] = {k: ((torch.from_numpy(lattice(v.shape)) + 0.0078125,
                            torch.from_numpy(np.abs(lattice(v.shape))) + 0.0078125) if moments else None)
                       for k, v in params.items()}
    return case


def assert_bands(case: dict, knobs: dict = KNOBS, rel: float = 1e-3) -> None:
    """No row within a relative `rel` of a threshold (opacity logit: 0.01 absolute)."""
    acc, den = case["accum"].double().reshape(-1), case["denom"].double().reshape(-1)
    g = acc / den
    fin = torch.isfinite(g)
    away = lambda v, t: bool(((v - t).abs() > rel * t).all())   # noqa: E731
    assert away(g[fin], knobs["max_grad"])
    ms = torch.exp(case["params"]["scaling"].double()).max(dim=1).values
    assert away(ms, knobs["percent_dense"] * knobs["extent"])
    assert away(ms, 0.1 * knobs["extent"]) and away(ms / 1.6, 0.1 * knobs["extent"])
    logit = math.log(knobs["min_opacity"] / (1 - knobs["min_opacity"]))
    assert bool(((case["params"]["opacity"].double() - logit).abs() >= 0.01).all())


def expected_classes(case: dict, max_screen_size, knobs: dict = KNOBS) -> dict:
    """Row counts per class, in float64: clone, split, pruned originals (unsplit rows the prune test drops),
    split rows whose children are pruned, rows with x / 0 = inf and with 0 / 0."""
    acc, den = case["accum"].double().reshape(-1), case["denom"].double().reshape(-1)
    g = torch.nan_to_num(acc / den, nan=0.0, posinf=float("inf"))
    ms = torch.exp(case["params"]["scaling"].double()).max(dim=1).values
    sel = g >= knobs["max_grad"]
    small = ms <= knobs["percent_dense"] * knobs["extent"]
    faint = torch.sigmoid(case["params"]["opacity"].double()).reshape(-1) < knobs["min_opacity"]
    big = ms > 0.1 * knobs["extent"] if max_screen_size else torch.zeros_like(faint)
    big_child = ms / 1.6 > 0.1 * knobs["extent"] if max_screen_size else torch.zeros_like(faint)
    split = sel & ~small
    return {"clone": int((sel & small).sum()), "split": int(split.sum()),
            "pruned_original": int((~split & (faint | big)).sum()),
            "pruned_child_parents": int((split & (faint | big_child)).sum()),
            "inf": int(((den == 0) & (acc > 0)).sum()), "nan": int(((den == 0) & (acc == 0)).sum())}
