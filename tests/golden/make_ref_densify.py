"""Generate tests/golden/ref_densify.npz by running the REFERENCE's own
GaussianModel.densify_and_prune and reset_opacity (scene/gaussian_model.py:303-306,
352-504) on the CPU.  Pins langsplatv2_amd/densify.py (tests/test_densify.py).

The reference's model runs unchanged, prepared as follows:
  * `plyfile` and `simple_knn._C` are stubbed in sys.modules (unused here);
  * scene/gaussian_model.py is loaded by file path (scene/__init__ pulls in cv2);
  * the device="cuda" keyword of torch.zeros / ones / empty is remapped to the CPU;
  * torch.normal(mean, std) is replaced by mean + std * z with the recorded z:
    noise (N, 2, 3) indexed by parent row and round, laid out round-major over the
    selected parents, as `.repeat(2, 1)` lays out std.

The inputs (tests/densify_cases.py, N = 400, SH degree 1) go through one real
Adam step of the reference's optimiser first, so the moments are non-zero and
`step` is 1.  Stored: the inputs after that step, the noise, the outputs of
densify_and_prune with max_screen_size None and 20, and of reset_opacity.

Run:  LSR_REFERENCE=<reference checkout> python tests/golden/make_ref_densify.py
(only the resulting .npz is committed and travels)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from densify_cases import GROUPS, KNOBS, assert_bands, make_case  # noqa: E402

if not os.environ.get("LSR_REFERENCE"):
    sys.exit("set LSR_REFERENCE to the reference checkout (the directory holding scene/gaussian_model.py)")
REF = os.environ["LSR_REFERENCE"]
OUT = os.path.join(HERE, "ref_densify.npz")
ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
N, SEED = 400, 5


def load_reference():
    sys.path.insert(0, REF)
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = None
    knn = types.ModuleType("simple_knn")
    knn_c = types.ModuleType("simple_knn._C")
    knn_c.distCUDA2 = None
    knn._C = knn_c
    sys.modules.update({"plyfile": ply, "simple_knn": knn, "simple_knn._C": knn_c})
    for name in ("zeros", "ones", "empty"):
        orig = getattr(torch, name)

        def on_cpu(*a, _orig=orig, **kw):
            if str(kw.get("device", "")).startswith("cuda"):
                kw["device"] = "cpu"
            return _orig(*a, **kw)
        setattr(torch, name, on_cpu)
    spec = importlib.util.spec_from_file_location("ref_gaussian_model", os.path.join(REF, "scene", "gaussian_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fresh_model(mod, case, grads):
    """A GaussianModel over the case's tensors after one Adam step with `grads`."""
    gm = mod.GaussianModel(1)
    for k, a in zip(GROUPS, ATTRS):
        setattr(gm, a, torch.nn.Parameter(case["params"][k].clone().requires_grad_(True)))
    gm.spatial_lr_scale = 1.0
    args = types.SimpleNamespace(percent_dense=KNOBS["percent_dense"], include_feature=False, position_lr_init=0.00016,
                                 position_lr_final=0.0000016, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
                                 feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
    gm.training_setup(args)
    for k, a in zip(GROUPS, ATTRS):
        getattr(gm, a).grad = grads[k].clone()
    gm.optimizer.step()
    gm.optimizer.zero_grad(set_to_none=True)
    gm.xyz_gradient_accum = case["accum"].clone()
    gm.denom = case["denom"].clone()
    gm.max_radii2D = case["max_radii2D"].clone()
    return gm


def snapshot(gm, prefix, out):
    groups = {g["name"]: g for g in gm.optimizer.param_groups}
    for k, a in zip(GROUPS, ATTRS):
        p = getattr(gm, a)
        assert groups[k]["params"][0] is p
        st = gm.optimizer.state[p]
        out[f"{prefix}_{k}"] = p.detach().numpy().copy()
        out[f"{prefix}_{k}_exp_avg"] = st["exp_avg"].numpy().copy()
        out[f"{prefix}_{k}_exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
        out[f"{prefix}_{k}_step"] = np.float32(float(st["step"]))
    out[f"{prefix}_accum"] = gm.xyz_gradient_accum.numpy().copy()
    out[f"{prefix}_denom"] = gm.denom.numpy().copy()
    out[f"{prefix}_max_radii2D"] = gm.max_radii2D.numpy().copy()


def main():
    mod = load_reference()
    case = make_case(N, SEED, coeffs=4)
    rng = np.random.default_rng(SEED + 1)
    grads = {k: torch.from_numpy(rng.choice([-0.5, -0.25, 0.125, 1.0], tuple(v.shape)).astype(np.float32))
             for k, v in case["params"].items()}
    out = {"noise": case["noise"].numpy()}
    snapshot(fresh_model(mod, case, grads), "in", out)
    stepped = dict(case, params={k: torch.from_numpy(out[f"in_{k}"]) for k in GROUPS})
    assert_bands(stepped)   # the step moved scaling by 0.005 and opacity by 0.05: still clear of every threshold

    real_normal = torch.normal
    for tag, mss in (("none", None), ("s20", 20)):
        gm = fresh_model(mod, case, grads)
        # the rows densify_and_split will select, in the reference's own expressions
        g = gm.xyz_gradient_accum / gm.denom
        g[g.isnan()] = 0.0
        sel = (g.squeeze() >= KNOBS["max_grad"]) & \
              (torch.max(gm.get_scaling, dim=1).values > gm.percent_dense * KNOBS["extent"])
        z = case["noise"][sel].permute(1, 0, 2).reshape(-1, 3)

        def recorded(mean, std, _z=z):
            assert tuple(std.shape) == tuple(_z.shape), (std.shape, _z.shape)
            return mean + std * _z
        torch.normal = recorded
        try:
            gm.densify_and_prune(KNOBS["max_grad"], KNOBS["min_opacity"], KNOBS["extent"], mss)
        finally:
            torch.normal = real_normal
        snapshot(gm, f"out_{tag}", out)
        out[f"out_{tag}_n_split"] = np.int64(int(sel.sum()))

    gm = fresh_model(mod, case, grads)
    gm.reset_opacity()
    snapshot(gm, "reset", out)
    out = {k: v for k, v in out.items() if not (k.startswith("reset_") and "opacity" not in k)}
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; rows", N, "->", out["out_none_xyz"].shape[0],
          out["out_s20_xyz"].shape[0])


if __name__ == "__main__":
    main()
