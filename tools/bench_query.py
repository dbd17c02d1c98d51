"""Text-query relevancy maps of the quick path on one MI355X: the fused kernel
(langsplatv2_amd.query.relevancy_maps) against the paths it replaces.

The reference renders the 192-channel weight map, decodes it against 3 x 64 x
512 codebooks, L2-normalises (eval_lerf.py:210-220) and hands the 512-d map to
OpenCLIPNetwork.get_max_across_quick (eval/openclip_encoder.py:114-139).
Synthetic: 1M Gaussians (SURVEY §8d generator), random codebooks, Q = 4
positives + 4 negatives, the rasterizer's default pixel-major map.  Timed, all
in one process and alternating, `--repeats` times `--iters` calls each, every
window closed by a device synchronise:

  a  relevancy_maps                                     (this kernel)
  b  decode_language_features alone                     (a strict part of c)
  c  decode_language_features + get_max_across_quick restated in torch
                                                        (what a caller had before)
  d  the all-torch consumer: einsum + norm + the same torch restatement
  r  the quick render;  ra  render then relevancy_maps, back to back

Prints one JSON line per resolution: the median and the repeat-to-repeat spread
(max - min) of each, render + relevancy as FPS, the kernel's algorithmic bytes
H*W*(768 + 4*L*Q) and the share of the HBM peak they amount to (the kernel's
bound is bandwidth: 768 B read per pixel and level set against ~250 split-f16
MFMAs per 64-pixel tile).

  python tools/bench_query.py [--iters 20] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from langsplatv2_amd import query, quick  # noqa: E402
from langsplatv2_amd.scenes import make_camera, make_gaussians  # noqa: E402

HBM_PEAK = 8.0e12        # B/s, datasheet
HBM_MEASURED = 6.29e12   # B/s, float4 copy


def torch_max_across_quick(sem_map, pos, neg, scale=10.0):
    """get_max_across_quick restated: sem_map (L, H, W, Df) -> (L, Q, H, W)."""
    L, H, W, C = sem_map.shape
    Q, N = pos.shape[0], neg.shape[0]
    flat = sem_map.permute(0, 3, 1, 2).reshape(L, C, -1).permute(0, 2, 1).contiguous()
    sim = torch.einsum("nqc,pc->nqp", flat, torch.cat([pos, neg], 0).to(sem_map.dtype))
    p = sim[:, :, :Q].unsqueeze(-1).repeat(1, 1, 1, N)
    n = sim[:, :, Q:].unsqueeze(2).repeat(1, 1, Q, 1)
    soft = torch.softmax(scale * torch.stack([p, n], dim=-1), dim=-1)
    return soft[..., 0].min(dim=-1)[0].permute(0, 2, 1).reshape(L, Q, H, W)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--sizes", default="1280x800,1920x1080")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_query.py needs a ROCm GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    L, K, Df, Q, N = 3, 64, 512, 4, 4
    gen = torch.Generator().manual_seed(0)
    cb = torch.randn(L, K, Df, generator=gen).to(dev)
    pos = torch.nn.functional.normalize(torch.randn(Q, Df, generator=gen), dim=-1).to(dev)
    neg = torch.nn.functional.normalize(torch.randn(N, Df, generator=gen), dim=-1).to(dev)
    for W, H in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        cam = make_camera(W, H)
        g = make_gaussians(args.gaussians, cam, seed=0, sh_degree=3, quick_k=4)
        t = {k: v.to(dev) for k, v in g.items() if isinstance(v, torch.Tensor)}
        rs = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
            bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam["viewmatrix"].to(dev),
            projmatrix=cam["projmatrix"].to(dev), sh_degree=3, campos=cam["campos"].to(dev), prefiltered=False,
            debug=False, include_feature=False, quick_render=True)
        r = GaussianRasterizer(rs)
        z = torch.zeros_like(t["means3D"])

        def render():
            with torch.no_grad():
                return r(means3D=t["means3D"], means2D=z, opacities=t["opacities"], shs=t["shs"],
                         language_feature_weights_quick=t["language_feature_weights_quick"],
                         language_feature_indices=t["language_feature_indices"], scales=t["scales"],
                         rotations=t["rotations"])[1]

        wmap = render()
        assert wmap.stride() == (1, L * K * W, L * K), "the default quick map is pixel-major"
        wchw = wmap.contiguous()   # the reference's (L*K, H, W) map, for its einsum

        def torch_decode():
            f = torch.einsum("ldk,lkn->ldn", cb.permute(0, 2, 1), wchw.view(L, K, H * W)).view(L, Df, H, W)
            return f / (f.norm(dim=1, keepdim=True) + 1e-10)

        fns = {
            "relevancy": lambda: query.relevancy_maps(wmap, cb, pos, neg),
            "decode": lambda: quick.decode_language_features(wmap, cb),
            "decode_torch_consumer": lambda: torch_max_across_quick(
                quick.decode_language_features(wmap, cb).permute(0, 2, 3, 1), pos, neg),
            "all_torch": lambda: torch_max_across_quick(torch_decode().permute(0, 2, 3, 1), pos, neg),
            "render": render,
            "render_relevancy": lambda: query.relevancy_maps(render(), cb, pos, neg),
        }
        slow = {"decode_torch_consumer", "all_torch"}
        # the fused kernel and the path it replaces compute the same maps
        dev_abs = float((fns["relevancy"]() - fns["decode_torch_consumer"]()).abs().max())
        for fn in fns.values():   # warm-up of every shape timed below
            fn()
            fn()
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                ms[k].append(window(fn, max(3, args.iters // 4) if k in slow else args.iters))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        nbytes = H * W * (L * K * 4 + 4 * L * Q)
        bps = nbytes / (med["relevancy"] * 1e-3)
        print(json.dumps({
            "workload": f"text-query relevancy, Q={Q} positives + {N} negatives, 3x64x512 codebooks, "
                        f"{args.gaussians} Gaussians, {W}x{H}, pixel-major map",
            "iters": args.iters, "repeats": args.repeats,
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_spread": {k: round(v, 4) for k, v in spread.items()},
            "relevancy_faster_than_decode_beyond_spread":
                max(ms["relevancy"]) + spread["relevancy"] + spread["decode"] < min(ms["decode"]),
            "decode_over_relevancy": round(med["decode"] / med["relevancy"], 2),
            "decode_torch_consumer_over_relevancy": round(med["decode_torch_consumer"] / med["relevancy"], 2),
            "render_relevancy_fps": round(1e3 / med["render_relevancy"], 1),
            "render_only_fps": round(1e3 / med["render"], 1),
            "relevancy_algorithmic_bytes": nbytes,
            "relevancy_GBps": round(bps / 1e9, 1),
            "relevancy_share_of_hbm_peak": {"bound": "bandwidth", "of_8.0TBps_spec": round(bps / HBM_PEAK, 3),
                                            "of_6.29TBps_measured_copy": round(bps / HBM_MEASURED, 3)},
            "max_abs_diff_vs_decode_torch_consumer": dev_abs}), flush=True)
        del wmap, wchw


if __name__ == "__main__":
    main()
