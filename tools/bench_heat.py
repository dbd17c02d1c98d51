"""Query heatmap frames of the viewer path on one MI355X: the fused maps and
colour stage (langsplatv2_amd.heatmap) against what a user composes without
them.

The reference's render server decodes all levels, sums the normalised level
features, renormalises, takes the cosine with the prompt, and on the host
gates, normalises, colours and blends (backend_renderer.py:204-233); its
prompt demo takes get_max_across_quick(...).mean(0), gates, normalises, raises
to the 4th power and colours (demo_prompt.py:122-137).  Synthetic: 1M
Gaussians (SURVEY §8d generator), random 3 x 64 x 512 codebooks, the
rasterizer's default pixel-major map and its RGB image; one prompt (the
server's case) and 4 prompts + 4 negatives.  Timed, all in one process and
alternating, `--repeats` times `--iters` calls each, every window closed by a
device synchronise:

  server_fused   summed_similarity_maps + heat_frames(rgb=...)
  server_parent  decode_language_features + the torch restatement of
                 backend_renderer.py:204-233 on the device (table by indexing)
  demo_fused     mean_relevancy_maps + heat_frames(curve="power4", min_range=0)
  demo_parent    relevancy_maps(...).mean(0) + the torch restatement of
                 demo_prompt.py:126-137 on the device
  summed_map, mean_map, frame   the new kernels alone
  decode         decode_language_features alone (k_quick_decode, which the map
                 kernel replaces: the map is expected to cost no more)

Writes the medians, the repeat-to-repeat spreads (max - min) and the byte
differences between the fused and the composed frames to --out, one record per
resolution and prompt count.

  python tools/bench_heat.py [--iters 20] [--repeats 5] [--out profiles/heat_bench.json]
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
from langsplatv2_amd import heatmap, query, quick  # noqa: E402
from langsplatv2_amd.scenes import make_camera, make_gaussians  # noqa: E402


def torch_colour(sim, lut, rgb, curve, threshold, min_range, alpha=0.5):
    """The servers' host tail on the device: sim (Q, H, W) -> (Q, H, W, 3) uint8."""
    frames = []
    for x in sim:
        mn, mx = x.min(), x.max()
        if curve == "upper_half":
            v = ((x - mn) / (mx - mn + 1e-9) * 2 - 1).clamp(0, 1)
        else:
            v = ((x - mn) / (mx - mn + 1e-8)) ** 4
        v = torch.where((mx < threshold) | (mx - mn < min_range), torch.zeros_like(v), v)
        heat = lut[(v * 255).to(torch.uint8).long()]
        if rgb is not None:
            final = rgb.permute(1, 2, 0) * (1 - alpha) + (heat.float() / 255.0) * alpha
            heat = (final.clamp(0, 1) * 255).to(torch.uint8)
        frames.append(heat)
    return torch.stack(frames)


def torch_summed(F, e):
    """backend_renderer.py:204-210 on the decoded (L, Df, H, W) map."""
    s = F.sum(dim=0)
    s = s / (s.norm(dim=0, keepdim=True) + 1e-10)
    return torch.einsum("dhw,qd->qhw", s, e)


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
    ap.add_argument("--out", default=os.path.join("profiles", "heat_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_heat.py needs a ROCm GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    L, K, Df = 3, 64, 512
    gen = torch.Generator().manual_seed(0)
    cb = torch.randn(L, K, Df, generator=gen).to(dev)
    # prompts along mixes of codebook rows, so the maps pass the gates and the colour stage does its full work
    mix = torch.einsum("qlk,lkd->qd", torch.rand(4, L, K, generator=gen), cb.cpu())
    pos4 = torch.nn.functional.normalize(torch.nn.functional.normalize(mix, dim=-1)
                                         + 0.5 * torch.randn(4, Df, generator=gen) / Df ** 0.5, dim=-1).to(dev)
    neg = torch.nn.functional.normalize(torch.randn(4, Df, generator=gen), dim=-1).to(dev)
    lut = heatmap.jet_lut(dev)
    records = []
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
        with torch.no_grad():
            res = r(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"],
                    shs=t["shs"], language_feature_weights_quick=t["language_feature_weights_quick"],
                    language_feature_indices=t["language_feature_indices"], scales=t["scales"],
                    rotations=t["rotations"])
        rgb, wmap = res[0].contiguous(), res[1]
        assert wmap.stride() == (1, L * K * W, L * K), "the default quick map is pixel-major"
        del t, g
        for Q in (1, 4):
            pos = pos4[:Q].contiguous()
            server = dict(curve="upper_half", threshold=0.22, min_range=0.02)
            demo = dict(curve="power4", threshold=0.22, min_range=0.0)
            maps = heatmap.summed_similarity_maps(wmap, cb, pos)
            fns = {
                "server_fused": lambda: heatmap.heat_frames(heatmap.summed_similarity_maps(wmap, cb, pos), lut,
                                                            rgb=rgb, **server),
                "server_parent": lambda: torch_colour(torch_summed(quick.decode_language_features(wmap, cb), pos),
                                                      lut, rgb, **server),
                "demo_fused": lambda: heatmap.heat_frames(heatmap.mean_relevancy_maps(wmap, cb, pos, neg), lut,
                                                          **demo),
                "demo_parent": lambda: torch_colour(query.relevancy_maps(wmap, cb, pos, neg).mean(0), lut, None,
                                                    **demo),
                "summed_map": lambda: heatmap.summed_similarity_maps(wmap, cb, pos),
                "mean_map": lambda: heatmap.mean_relevancy_maps(wmap, cb, pos, neg),
                "frame": lambda: heatmap.heat_frames(maps, lut, rgb=rgb, **server),
                "decode": lambda: quick.decode_language_features(wmap, cb),
            }
            slow = {"server_parent", "demo_parent"}
            # the fused frames against the composed ones: the maps agree to ~1e-7, so a byte moves only
            # where a value sits on a rounding edge
            diff = {}
            for a, b in (("server_fused", "server_parent"), ("demo_fused", "demo_parent")):
                d = (fns[a]().int() - fns[b]().int()).abs()
                diff[a] = {"max_byte_diff": int(d.max()), "share_of_bytes_differing": float((d > 0).float().mean())}
            live = float((maps.amax(dim=(1, 2)) >= 0.22).float().mean())
            for fn in fns.values():   # warm-up of every shape timed below
                fn()
                fn()
            ms = {k: [] for k in fns}
            for _ in range(args.repeats):
                for k, fn in fns.items():
                    ms[k].append(window(fn, max(3, args.iters // 4) if k in slow else args.iters))
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: max(v) - min(v) for k, v in ms.items()}
            rec = {
                "workload": f"query heatmap frames, Q={Q} prompts (+ 4 negatives for the demo), 3x64x512 codebooks, "
                            f"{args.gaussians} Gaussians, {W}x{H}, pixel-major map",
                "iters": args.iters, "repeats": args.repeats,
                "ms_median": {k: round(v, 4) for k, v in med.items()},
                "ms_spread": {k: round(v, 4) for k, v in spread.items()},
                "server_parent_over_fused": round(med["server_parent"] / med["server_fused"], 2),
                "demo_parent_over_fused": round(med["demo_parent"] / med["demo_fused"], 2),
                "summed_map_over_decode": round(med["summed_map"] / med["decode"], 3),
                "summed_map_no_slower_than_decode_beyond_spread":
                    min(ms["summed_map"]) - spread["summed_map"] - spread["decode"] <= max(ms["decode"]),
                "share_of_prompts_passing_the_gate": live,
                "frames_vs_parent": diff}
            print(json.dumps(rec), flush=True)
            records.append(rec)
        del wmap, rgb
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
