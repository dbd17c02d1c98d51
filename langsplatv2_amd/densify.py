"""Adaptive density control of the RGB phase, fused on the GPU.

The reference's `GaussianModel.densify_and_prune` (scene/gaussian_model.py:352-504,
run every 100 iterations up to 15,000: train.py:246-258) clones small Gaussians
with a large view-space gradient, splits large ones into two sampled children,
and prunes faint or oversized ones -- as three passes of boolean-index gathers
and `cat`s over the six parameter tensors and their twelve Adam moments.  Its
result is four stably compacted segments of the input rows:

  1. originals that were neither split nor pruned      (moments copied)
  2. clones that pass the prune test                   (moments zero)
  3. round-0 children that pass the prune test         (moments zero)
  4. round-1 children, likewise

`densify_tensors` computes exactly that with a plan (classify, scan, fill: one
host read-back of the segment sizes) and one gather launch for all 18 tensors
(csrc/densify.hip, C ABI lsr_densify_plan / lsr_densify_apply).
`densify_and_prune` applies it to a `train_loop.GaussianState` and its optimiser
(FusedAdam or torch.optim.Adam), `reset_opacity` is the reference's method of
that name, and `densify_and_prune_torch` restates the reference's op sequence
in torch (any device and dtype, explicit noise): the checker and the A/B
baseline (`fused=False`).

Kept as the reference has it: `densification_postfix` zeroes `max_radii2D`
before the final prune, so the `max_radii2D > max_screen_size` term never
fires.  `max_radii2D` is accepted for interface parity and has no effect;
`max_screen_size` only switches the `max exp(scaling) > 0.1 * extent` test on.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import torch

from . import _lib

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")

DensifyResult = namedtuple("DensifyResult", "n_before n_clone n_split n_pruned n_after")
DensifyResult.__doc__ = """Row counts of one densify_and_prune: rows selected for cloning and for splitting
(a split replaces its row by two children), rows the prune test removed (originals, clones and children
alike), so n_after = n_before + n_clone + n_split - n_pruned."""


def _check_args(params, moments, accum, denom, max_radii2D, max_grad, noise, who, fused):
    if not max_grad > 0:
        raise ValueError(f"{who}: max_grad must be > 0 (a clone's padded gradient is 0 and must not be selected "
                         f"for a split), got {max_grad}")
    missing = [k for k in GROUPS if k not in params]
    if missing:
        raise ValueError(f"{who}: params lacks {missing}")
    n = params["xyz"].shape[0]
    want = {"xyz": (n, 3), "f_dc": (n, 1, 3), "opacity": (n, 1), "scaling": (n, 3), "rotation": (n, 4)}
    rest = params["f_rest"]
    if rest.dim() != 3 or rest.shape[0] != n or rest.shape[2] != 3:
        raise ValueError(f"{who}: f_rest must be (N, M - 1, 3), got {tuple(rest.shape)}")
    for k, shp in want.items():
        if tuple(params[k].shape) != shp:
            raise ValueError(f"{who}: {k} must be {shp}, got {tuple(params[k].shape)}")
    tensors = [(k, params[k]) for k in GROUPS]
    for k in GROUPS:
        mom = moments.get(k) if moments is not None else None
        if mom is None:
            continue
        if len(mom) != 2:
            raise ValueError(f"{who}: moments[{k!r}] must be (exp_avg, exp_avg_sq) or None")
        for nm, t in zip(("exp_avg", "exp_avg_sq"), mom):
            if tuple(t.shape) != tuple(params[k].shape):
                raise ValueError(f"{who}: {nm} of {k} is {tuple(t.shape)}, the parameter {tuple(params[k].shape)}")
            tensors.append((f"{k}.{nm}", t))
    for nm, t, shapes in (("xyz_gradient_accum", accum, ((n, 1), (n,))), ("denom", denom, ((n, 1), (n,))),
                          ("max_radii2D", max_radii2D, ((n,),))):
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{who}: {nm} must be {' or '.join(map(str, shapes))}, got {tuple(t.shape)}")
    tensors += [("xyz_gradient_accum", accum), ("denom", denom)]
    if noise is not None:
        if tuple(noise.shape) != (n, 2, 3):
            raise ValueError(f"{who}: noise must be (N, 2, 3) = {(n, 2, 3)}, got {tuple(noise.shape)}")
        tensors.append(("noise", noise))
    if fused:
        for nm, t in tensors:   # the C ABI takes raw pointers
            if t.dtype != torch.float32:
                raise ValueError(f"{who}: {nm} must be float32, got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"{who}: {nm} must be contiguous")
        for nm, t in tensors:
            if not t.is_cuda:
                raise RuntimeError(f"{who}: {nm} must be a ROCm device tensor (there is no CPU path; "
                                   "densify_and_prune_torch runs anywhere)")
    return n


def _result(n_before, n_clone, n_split, n_after):
    return DensifyResult(n_before, n_clone, n_split, n_before + n_clone + n_split - n_after, n_after)


def densify_tensors(params: dict, moments: dict | None, accum: torch.Tensor, denom: torch.Tensor,
                    max_radii2D: torch.Tensor, *, max_grad: float, min_opacity: float, extent: float,
                    max_screen_size, percent_dense: float = 0.01, noise: torch.Tensor | None = None,
                    generator: torch.Generator | None = None):
    """densify_and_prune(max_grad, min_opacity, extent, max_screen_size) as a function of tensors.

    params: {name: tensor} for the reference's groups xyz (N, 3), f_dc (N, 1, 3), f_rest (N, M - 1, 3),
    opacity (N, 1), scaling (N, 3), rotation (N, 4); moments: {name: (exp_avg, exp_avg_sq) or None} (None:
    the optimiser has no state for that group yet); accum / denom (N, 1), max_radii2D (N,) (no effect, see
    the module docstring).  noise: standard-normal (N, 2, 3) indexed by parent row and round; None draws it
    with torch.randn(..., generator=generator) on the device.  All fp32, contiguous, on one ROCm device.

    Returns (params, moments, (xyz_gradient_accum, denom, max_radii2D), DensifyResult): new tensors, the
    statistics as zeros of the new length."""
    who = "densify_tensors"
    n = _check_args(params, moments, accum, denom, max_radii2D, max_grad, noise, who, fused=True)
    dev = params["xyz"].device
    if noise is None:
        noise = torch.randn((n, 2, 3), dtype=torch.float32, device=dev, generator=generator)
    lib = _lib.load()
    from .rasterizer import _stream
    stream = _stream(dev)
    counts = (ctypes.c_int64 * 6)()
    ws = None
    if n > 0:
        with torch.cuda.device(dev):
            ws = torch.empty(lib.lsr_densify_workspace_bytes(n), dtype=torch.uint8, device=dev)
            # thresholds as the reference's fp32 comparisons see them: Python doubles rounded once to fp32
            _lib.check(lib.lsr_densify_plan(n, accum.data_ptr(), denom.data_ptr(), params["scaling"].data_ptr(),
                                            params["opacity"].data_ptr(), float(max_grad),
                                            float(percent_dense * extent), float(min_opacity),
                                            1 if max_screen_size else 0, float(0.1 * extent), ws.data_ptr(), counts,
                                            stream), "lsr_densify_plan")
    n_out = int(counts[0] + counts[1] + counts[2] + counts[3])
    out_p = {k: torch.empty((n_out,) + tuple(params[k].shape[1:]), dtype=torch.float32, device=dev) for k in GROUPS}
    out_m = {}
    for k in GROUPS:
        mom = moments.get(k) if moments is not None else None
        out_m[k] = None if mom is None else (torch.empty_like(out_p[k]), torch.empty_like(out_p[k]))
    if n > 0 and n_out > 0:
        src = (ctypes.c_void_p * 18)()
        dst = (ctypes.c_void_p * 18)()
        for g, k in enumerate(GROUPS):
            src[g], dst[g] = params[k].data_ptr(), out_p[k].data_ptr()
            if out_m[k] is not None:
                for part in (0, 1):
                    src[6 * (part + 1) + g] = moments[k][part].data_ptr()
                    dst[6 * (part + 1) + g] = out_m[k][part].data_ptr()
        with torch.cuda.device(dev):
            _lib.check(lib.lsr_densify_apply(n, n_out, ws.data_ptr(), int(params["f_rest"].shape[1]) * 3, src, dst,
                                             noise.data_ptr(), stream), "lsr_densify_apply")
    stats = (torch.zeros((n_out, 1), device=dev), torch.zeros((n_out, 1), device=dev), torch.zeros((n_out,), device=dev))
    return out_p, out_m, stats, _result(n, int(counts[4]), int(counts[5]), n_out)


def build_rotation(r: torch.Tensor) -> torch.Tensor:
    """utils/general_utils.py:78-99 on r's device and dtype."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device, dtype=r.dtype)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


@torch.no_grad()
def densify_and_prune_torch(params: dict, moments: dict | None, accum: torch.Tensor, denom: torch.Tensor,
                            max_radii2D: torch.Tensor, *, max_grad: float, min_opacity: float, extent: float,
                            max_screen_size, percent_dense: float = 0.01, noise: torch.Tensor):
    """The reference's op sequence (densify_and_clone, densify_and_split, prune_points with
    cat_tensors_to_optimizer / _prune_optimizer; scene/gaussian_model.py:367-504) on plain tensors of any
    device and dtype, with `torch.normal(mean=0, std=stds)` replaced by `0 + stds * z` for the recorded
    z = noise (N, 2, 3) and the 3x3 `bmm` written as a left-to-right dot (the order the fused kernel uses).
    Same arguments and return value as densify_tensors."""
    _check_args(params, moments, accum, denom, max_radii2D, max_grad, noise, "densify_and_prune_torch", fused=False)
    P = {k: params[k].detach() for k in GROUPS}
    M = {k: (None if moments is None or moments.get(k) is None else [t.detach() for t in moments[k]]) for k in GROUPS}
    dev, dt = P["xyz"].device, P["xyz"].dtype
    n_before = P["xyz"].shape[0]
    accum, denom = accum.reshape(n_before, 1), denom.reshape(n_before, 1)

    def cat(ext):   # cat_tensors_to_optimizer + densification_postfix
        for k in GROUPS:
            if M[k] is not None:
                M[k] = [torch.cat((m, torch.zeros_like(ext[k])), dim=0) for m in M[k]]
            P[k] = torch.cat((P[k], ext[k]), dim=0)

    def prune(mask):   # prune_points
        valid = ~mask
        for k in GROUPS:
            if M[k] is not None:
                M[k] = [m[valid] for m in M[k]]
            P[k] = P[k][valid]

    grads = accum / denom
    grads[grads.isnan()] = 0.0
    # densify_and_clone
    sel = torch.where(torch.norm(grads, dim=-1) >= max_grad, True, False)
    sel = torch.logical_and(sel, torch.max(torch.exp(P["scaling"]), dim=1).values <= percent_dense * extent)
    n_clone = int(sel.sum())
    cat({k: P[k][sel] for k in GROUPS})
    # densify_and_split (N = 2)
    n_init = P["xyz"].shape[0]
    padded = torch.zeros((n_init,), device=dev, dtype=dt)
    padded[:n_before] = grads.squeeze(-1)
    sel = torch.where(padded >= max_grad, True, False)
    sel = torch.logical_and(sel, torch.max(torch.exp(P["scaling"]), dim=1).values > percent_dense * extent)
    n_split = int(sel.sum())
    stds = torch.exp(P["scaling"])[sel].repeat(2, 1)
    means = torch.zeros((stds.size(0), 3), device=dev, dtype=dt)
    z = noise.to(dt)[sel[:n_before]].permute(1, 0, 2).reshape(-1, 3)   # round-major, as .repeat(2, 1) lays the parents out
    samples = means + stds * z
    rots = build_rotation(P["rotation"][sel]).repeat(2, 1, 1)
    # bmm(rots, samples) written out as the left-to-right three-term dot: a library bmm may fuse or reorder
    # the sum depending on the CPU it runs on, and the golden file must compare equal on any machine
    rotated = (rots[:, :, 0] * samples[:, 0:1] + rots[:, :, 1] * samples[:, 1:2]) + rots[:, :, 2] * samples[:, 2:3]
    new = {"xyz": rotated + P["xyz"][sel].repeat(2, 1),
           "scaling": torch.log(torch.exp(P["scaling"])[sel].repeat(2, 1) / (0.8 * 2)),
           "rotation": P["rotation"][sel].repeat(2, 1),
           "f_dc": P["f_dc"][sel].repeat(2, 1, 1),
           "f_rest": P["f_rest"][sel].repeat(2, 1, 1),
           "opacity": P["opacity"][sel].repeat(2, 1)}
    cat(new)
    prune(torch.cat((sel, torch.zeros(2 * n_split, device=dev, dtype=torch.bool))))
    # the final prune; max_radii2D was zeroed by densification_postfix, so its term is always False
    radii = torch.zeros((P["xyz"].shape[0],), device=dev, dtype=dt)
    mask = (torch.sigmoid(P["opacity"]) < min_opacity).squeeze(-1)
    if max_screen_size:
        big_vs = radii > max_screen_size
        big_ws = torch.exp(P["scaling"]).max(dim=1).values > 0.1 * extent
        mask = torch.logical_or(torch.logical_or(mask, big_vs), big_ws)
    prune(mask)
    n_after = P["xyz"].shape[0]
    stats = (torch.zeros((n_after, 1), device=dev, dtype=dt), torch.zeros((n_after, 1), device=dev, dtype=dt),
             torch.zeros((n_after,), device=dev, dtype=dt))
    return P, {k: (None if M[k] is None else tuple(M[k])) for k in GROUPS}, stats, \
        _result(n_before, n_clone, n_split, n_after)


def _groups_by_name(opt) -> dict:
    groups = {g.get("name"): g for g in opt.param_groups}
    for k in GROUPS:
        if k not in groups or len(groups[k]["params"]) != 1:
            raise ValueError(f"densify: the optimiser needs one single-parameter group named {k!r}")
    return groups


def _rebind(gs, opt, groups, name, attr, new, exp_avg=None, exp_avg_sq=None):
    """Replace the group's parameter by the leaf `new` and move its state entry to it (the reference's
    _prune_optimizer / cat_tensors_to_optimizer / replace_tensor_to_optimizer); `step` is kept."""
    group = groups[name]
    old = group["params"][0]
    state = opt.state.get(old, None)
    new = new.requires_grad_(True)
    if state is not None and len(state) > 0:
        state["exp_avg"], state["exp_avg_sq"] = exp_avg, exp_avg_sq
        del opt.state[old]
        group["params"][0] = new
        opt.state[new] = state
    else:
        if old in opt.state:
            del opt.state[old]
        group["params"][0] = new
    setattr(gs, attr, new)


def _moments_of(opt, groups) -> dict:
    out = {}
    for k in GROUPS:
        st = opt.state.get(groups[k]["params"][0], None)
        out[k] = (st["exp_avg"], st["exp_avg_sq"]) if st is not None and "exp_avg" in st else None
    return out


@torch.no_grad()
def densify_and_prune(gs, opt, *, max_grad: float, min_opacity: float, extent: float, max_screen_size,
                      percent_dense: float = 0.01, noise: torch.Tensor | None = None,
                      generator: torch.Generator | None = None, fused: bool = True) -> DensifyResult:
    """GaussianModel.densify_and_prune on a train_loop.GaussianState and its optimiser (FusedAdam or
    torch.optim.Adam with the reference's named groups): the six tensors become new leaves (their .grad is
    gone, as in the reference, so the optimiser step of this iteration skips them), param_groups and the
    state entries follow, and xyz_gradient_accum / denom / max_radii2D are zeros of the new length.
    fused=False runs densify_and_prune_torch on the same inputs instead."""
    groups = _groups_by_name(opt)
    params = {k: getattr(gs, a).detach() for k, a in zip(GROUPS, _ATTRS)}
    for k in GROUPS:
        if groups[k]["params"][0] is not getattr(gs, _ATTRS[GROUPS.index(k)]):
            raise ValueError(f"densify_and_prune: group {k!r} of the optimiser does not hold the state's tensor")
    moments = _moments_of(opt, groups)
    n = params["xyz"].shape[0]
    if noise is None:
        noise = torch.randn((n, 2, 3), dtype=torch.float32, device=params["xyz"].device, generator=generator)
    fn = densify_tensors if fused else densify_and_prune_torch
    out_p, out_m, stats, res = fn(params, moments, gs.xyz_gradient_accum, gs.denom, gs.max_radii2D, max_grad=max_grad,
                                  min_opacity=min_opacity, extent=extent, max_screen_size=max_screen_size,
                                  percent_dense=percent_dense, noise=noise)
    for k, a in zip(GROUPS, _ATTRS):
        m = out_m[k] if out_m[k] is not None else (None, None)
        _rebind(gs, opt, groups, k, a, out_p[k].contiguous(), *(None if t is None else t.contiguous() for t in m))
    gs.xyz_gradient_accum, gs.denom, gs.max_radii2D = stats
    return res


@torch.no_grad()
def reset_opacity(gs, opt, fused: bool = True) -> None:
    """GaussianModel.reset_opacity (scene/gaussian_model.py:303-306): opacity =
    inverse_sigmoid(min(sigmoid(opacity), 0.01)) as a new leaf, both moments zero, `step` kept."""
    groups = _groups_by_name(opt)
    old = gs._opacity
    st = opt.state.get(groups["opacity"]["params"][0], None)
    has_state = st is not None and "exp_avg" in st
    if fused:
        if not old.is_cuda or old.dtype != torch.float32:
            raise RuntimeError("reset_opacity: opacity must be an fp32 ROCm device tensor (fused=False runs anywhere)")
        from .rasterizer import _stream
        new = old.detach().clone(memory_format=torch.contiguous_format)
        m = torch.empty_like(new) if has_state else None
        v = torch.empty_like(new) if has_state else None
        with torch.cuda.device(new.device):
            _lib.check(_lib.load().lsr_reset_opacity(new.numel(), new.data_ptr(), m.data_ptr() if has_state else None,
                                                     v.data_ptr() if has_state else None, _stream(new.device)),
                       "lsr_reset_opacity")
    else:
        p = torch.min(torch.sigmoid(old.detach()), torch.ones_like(old) * 0.01)
        new = torch.log(p / (1 - p))
        m = torch.zeros_like(new) if has_state else None
        v = torch.zeros_like(new) if has_state else None
    _rebind(gs, opt, groups, "opacity", "_opacity", new, m, v)


__all__ = ["DensifyResult", "densify_tensors", "densify_and_prune", "densify_and_prune_torch", "reset_opacity",
           "build_rotation", "GROUPS"]
