"""Open-vocabulary label maps of the quick path on one MI355X: the fused kernel
(langsplatv2_amd.semantic.semantic_maps) against the paths it replaces.

The reference renders the 192-channel weight map, decodes it against 3 x 64 x
512 codebooks, L2-normalises (eval_lerf.py:210-220) and hands the 512-d map to
OpenCLIPNetwork.get_semantic_map (eval/openclip_encoder.py:82-94).  Synthetic:
1M Gaussians (SURVEY §8d generator), random codebooks, (C, N) = (21, 4) and
(150, 4) label sets, the rasterizer's pixel-major map and its (L*K, H, W) copy.
Timed, all in one process and alternating, `--repeats` times `--iters` calls
each, every window closed by a device synchronise:

  labels / labels_scores  semantic_maps per (C, N) and layout    (this kernel)
  a  decode_language_features + get_semantic_map restated in torch
                                                       (what a caller had before)
  b  relevancy_maps at Q = 4, N = 4, against semantic_maps at (4, 4) columns with
     scores: the same bytes read, fewer written
  merge / confusion       merge_levels, label_confusion on the (21, 4) maps

Prints one JSON line per resolution: the median and the repeat-to-repeat spread
(max - min) of each, the kernel's algorithmic bytes H*W*L*(768 + 4 or 8) and the
share of the HBM peak they amount to at (21, 4) (one 16-column block more than
the relevancy kernel's: bandwidth-bound like it; at 154 columns the ten blocks
of MFMAs and, with scores, exponentials per tile weigh in).

  python tools/bench_semantic.py [--iters 50] [--repeats 5] [--out profiles/semantic_bench.json]
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
from langsplatv2_amd import query, quick, semantic  # noqa: E402
from langsplatv2_amd.scenes import make_camera, make_gaussians  # noqa: E402

HBM_PEAK = 8.0e12        # B/s, datasheet
HBM_MEASURED = 6.29e12   # B/s, float4 copy (the rate DESIGN.md sets k_quick_query against)
SETS = [(21, 4), (150, 4)]


def torch_semantic_map(sem_map, sem, neg):
    """get_semantic_map restated: sem_map (L, H, W, Df) contiguous -> (L, H, W) int64."""
    L, H, W, C = sem_map.shape
    p = torch.cat([sem, neg], 0).to(sem_map.dtype)
    pred = torch.zeros(L, H, W, device=sem_map.device)
    for i in range(L):
        soft = torch.softmax(10 * torch.mm(sem_map[i].view(-1, C), p.T), dim=-1)
        pred[i] = torch.argmax(soft, dim=-1).view(H, W)
        pred[i][pred[i] >= sem.shape[0]] = -1
    return pred.long()


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--sizes", default="1280x800,1920x1080")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_semantic.py needs a ROCm GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    L, K, Df = 3, 64, 512
    gen = torch.Generator().manual_seed(0)
    cb = torch.randn(L, K, Df, generator=gen).to(dev)

    def units(n):
        return torch.nn.functional.normalize(torch.randn(n, Df, generator=gen), dim=-1).to(dev)

    neg = units(4)
    pos4 = units(4)
    labs = {C: units(C) for C, _ in SETS}
    lines = []
    for W, H in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        cam = make_camera(W, H)
        g = make_gaussians(args.gaussians, cam, seed=0, sh_degree=3, quick_k=4)
        t = {k: v.to(dev) for k, v in g.items() if isinstance(v, torch.Tensor)}
        rs = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
            bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam["viewmatrix"].to(dev),
            projmatrix=cam["projmatrix"].to(dev), sh_degree=3, campos=cam["campos"].to(dev), prefiltered=False,
            debug=False, include_feature=False, quick_render=True)
        with torch.no_grad():
            wmap = GaussianRasterizer(rs)(
                means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], shs=t["shs"],
                language_feature_weights_quick=t["language_feature_weights_quick"],
                language_feature_indices=t["language_feature_indices"], scales=t["scales"],
                rotations=t["rotations"])[1]
        assert wmap.stride() == (1, L * K * W, L * K), "the default quick map is pixel-major"
        maps = {"hwc": wmap, "chw": wmap.contiguous()}
        del t, g

        fns, slow = {}, set()
        for C, N in SETS:
            for lay, m in maps.items():
                fns[f"labels_{C}_{N}_{lay}"] = lambda m=m, C=C: semantic.semantic_maps(m, cb, labs[C], neg)
                fns[f"labels_scores_{C}_{N}_{lay}"] = lambda m=m, C=C: semantic.semantic_maps(m, cb, labs[C], neg,
                                                                                               with_scores=True)
            fns[f"a_decode_torch_{C}_{N}"] = lambda C=C: torch_semantic_map(
                quick.decode_language_features(wmap, cb).permute(0, 2, 3, 1).contiguous(), labs[C], neg)
            slow.add(f"a_decode_torch_{C}_{N}")
        fns["labels_scores_4_4_hwc"] = lambda: semantic.semantic_maps(wmap, cb, pos4, neg, with_scores=True)
        fns["b_relevancy_4_4_hwc"] = lambda: query.relevancy_maps(wmap, cb, pos4, neg)
        lab21, sco21 = semantic.semantic_maps(wmap, cb, labs[21], neg, with_scores=True)
        gt = lab21[0].clone()
        fns["merge_levels"] = lambda: semantic.merge_levels(lab21, sco21)
        fns["confusion_21_P3"] = lambda: semantic.label_confusion(lab21, gt, 21)

        # the fused kernel and the path it replaces give the same labels but for near-ties
        differ = {}
        for C, N in SETS:
            a = fns[f"a_decode_torch_{C}_{N}"]()
            differ[f"{C}_{N}"] = float((a != fns[f"labels_{C}_{N}_hwc"]().long()).float().mean())
            assert torch.equal(fns[f"labels_{C}_{N}_hwc"](), fns[f"labels_scores_{C}_{N}_chw"]()[0])
            del a
        for fn in fns.values():   # warm-up of every shape timed below
            fn()
            fn()
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                ms[k].append(window(fn, max(3, args.iters // 10) if k in slow else args.iters))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        sem44, rel44 = "labels_scores_4_4_hwc", "b_relevancy_4_4_hwc"
        nbytes = {"labels": H * W * L * (K * 4 + 4), "labels_scores": H * W * L * (K * 4 + 8)}
        bps = nbytes["labels_scores"] / (med["labels_scores_21_4_hwc"] * 1e-3)
        line = {
            "workload": f"semantic label maps, 3x64x512 codebooks, {args.gaussians} Gaussians, {W}x{H}, "
                        "(C, N) = (21, 4) and (150, 4), pixel-major (hwc) and (L*K, H, W) (chw) maps",
            "iters": args.iters, "repeats": args.repeats,
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_spread": {k: round(v, 4) for k, v in spread.items()},
            "a_over_labels": {f"{C}_{N}": round(med[f"a_decode_torch_{C}_{N}"] / med[f"labels_{C}_{N}_hwc"], 1)
                              for C, N in SETS},
            "semantic_4_4_minus_relevancy_4_4_ms": round(med[sem44] - med[rel44], 4),
            "semantic_4_4_slower_than_relevancy_beyond_spread":
                min(ms[sem44]) > max(ms[rel44]) + spread[sem44] + spread[rel44],
            "algorithmic_bytes": nbytes,
            "labels_scores_21_4_hwc_GBps": round(bps / 1e9, 1),
            "labels_scores_21_4_hwc_share_of_hbm_peak": {"bound": "bandwidth", "of_8.0TBps_spec": round(bps / HBM_PEAK, 3),
                                                         "of_6.29TBps_measured_copy": round(bps / HBM_MEASURED, 3)},
            "label_share_differing_from_a": differ}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del wmap, maps, fns, lab21, sco21, gt
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
