"""SAM mask NMS and segment maps (langsplatv2_amd.mask_nms, csrc/mask_nms.hip) at
N = 128 and 384 masks, 1280 x 800 and 1920 x 1080, on rectangle scenes from the
fixture generator (tests/golden/make_ref_mask_nms.py) with the reference's
call-site thresholds.

  python tools/bench_mask_nms.py [--iters 10] [--out profiles/mask_nms_bench.json] [--reference <checkout>]

Per shape, one JSON line per variant (ms, best of 3 alternating rounds, host clock
around work that ends in a device synchronise):
  hip            pack, pair counts, select (pair counts + decide; decide is the
                 difference), segment maps of four levels, and end to end
                 (pack + sort + select + count read-back + segment maps);
                 floors: the pack kernel's input bytes (N H W) per second, the
                 pair kernel's word-ANDs per second over the pairs it must do
                 (N (N + 1) / 2 x ceil(H W / 64)) and over the 64 x 64 tiles it runs
  torch          baseline (a), what a user would write on the same GPU:
                 masks.float().flatten(1) matmul for the intersections, then the
                 vectorised decision
  host_loop      baseline (b), the reference's Python double loop on the host at
                 N = 32 and the same frame: seconds per pair measured; the time
                 for all N (N + 1) / 2 pairs is labelled as extrapolated.  With
                 --reference the reference's own function, else its steps restated.
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MN = importlib.import_module("langsplatv2_amd.mask_nms")  # noqa: E402

SITE = dict(iou_thr=0.8, score_thr=0.7, inner_thr=0.5)
SHAPES = [(128, 800, 1280), (384, 800, 1280), (128, 1080, 1920), (384, 1080, 1920)]
HOST_N = 32


def maker():
    spec = importlib.util.spec_from_file_location("make_ref_mask_nms",
                                                  os.path.join(ROOT, "tests", "golden", "make_ref_mask_nms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scene(N, H, W, dev, seed=0):
    """The generator's boxes, rasterised on the device: (N, H, W) bool, (N,) float64."""
    boxes, scores = maker().rect_boxes(N, H, W, seed)
    b = torch.from_numpy(boxes).to(dev)
    ys = torch.arange(H, device=dev)[None, :, None]
    xs = torch.arange(W, device=dev)[None, None, :]
    masks = (ys >= b[:, 0, None, None]) & (ys < b[:, 1, None, None]) & (xs >= b[:, 2, None, None]) & (xs < b[:, 3, None, None])
    return masks.contiguous(), torch.from_numpy(scores).to(dev)


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def torch_pairs(masks, idx):
    m = masks[idx].float().flatten(1)
    return m @ m.T


def torch_decide(inter, ranked, idx, iou_thr, score_thr, inner_thr):
    """preprocess.py:242-279 on the whole table at once."""
    N = inter.shape[0]
    area = inter.diagonal()
    iou = inter / (area[:, None] + area[None, :] - inter)
    a, b = inter / area[:, None], inter / area[None, :]
    inner = 1 - b * a
    upper = torch.ones(N, N, dtype=torch.bool, device=inter.device).triu(1)
    zero = torch.zeros((), device=inter.device)
    mat = torch.where(upper & (a < 0.5) & (b >= 0.85), inner, zero) + \
        torch.where(upper & (a >= 0.85) & (b < 0.5), inner, zero).T
    keep = torch.triu(iou, 1).max(dim=0).values <= iou_thr
    crit = [ranked > score_thr, torch.triu(mat, 1).max(dim=0).values <= 1 - inner_thr,
            torch.tril(mat, 1).max(dim=0).values <= 1 - inner_thr]
    for k in crit:
        if k.sum() == 0:
            k[:3] = True
        keep = keep & k
    return idx[keep]


def host_pair_loop(masks, reference):
    """Seconds per pair of the reference's loop over HOST_N masks on the host."""
    n = masks.shape[0]
    pairs = n * (n + 1) // 2
    if reference:
        fn = maker().reference_mask_nms(reference)
        scores = torch.linspace(1.0, 0.4, n, dtype=torch.float64)
        t0 = time.perf_counter()
        fn(masks, scores, **SITE)
        return (time.perf_counter() - t0) / pairs, "reference function"
    area = torch.sum(masks, dim=(1, 2), dtype=torch.float)
    t0 = time.perf_counter()
    for i in range(n):       # its per-pair work restated: two full-frame reductions, the ratios
        for j in range(i, n):
            inter = torch.sum(torch.logical_and(masks[i], masks[j]), dtype=torch.float)
            union = torch.sum(torch.logical_or(masks[i], masks[j]), dtype=torch.float)
            _ = inter / union, inter / area[i] < 0.5, inter / area[j] >= 0.85, inter / area[i] >= 0.85, inter / area[j] < 0.5
    return (time.perf_counter() - t0) / pairs, "restated steps"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", default=os.environ.get("LSR_REFERENCE"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mask_nms: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    lines = []
    host_done = {}
    for N, H, W in SHAPES:
        masks, scores = scene(N, H, W, dev)
        W64 = (H * W + 63) // 64
        packed = MN.pack_masks(masks)
        ranked, idx = torch.sort(scores, descending=True, stable=True)
        res = MN.mask_nms(packed, scores, return_detail=True, **SITE)
        want = torch_decide(torch_pairs(masks, idx), ranked, idx, **SITE)
        pairs_equal = bool(torch.equal(res.inter.float().triu(), torch_pairs(masks, idx).triu()))
        keeps = [torch.sort(res.selected).values] * 4
        runs = {k: [] for k in ("pack", "pairs", "select", "segmaps", "end_to_end", "torch_pairs", "torch_decide",
                                "torch_nms")}
        inter_t = torch_pairs(masks, idx)

        def end_to_end():
            p = MN.pack_masks(masks)
            sel = MN.mask_nms(p, scores, **SITE)
            MN.build_seg_maps([p] * 4, [torch.sort(sel).values] * 4)

        for _ in range(3):   # alternate the variants so a busy neighbour hits both alike
            runs["pack"].append(timed(lambda: MN.pack_masks(masks), a.iters))
            runs["torch_pairs"].append(timed(lambda: torch_pairs(masks, idx), a.iters))
            runs["pairs"].append(timed(lambda: MN.mask_pair_counts(packed, idx), a.iters))
            runs["torch_decide"].append(timed(lambda: torch_decide(inter_t, ranked, idx, **SITE), a.iters))
            runs["select"].append(timed(lambda: MN.mask_nms(packed, scores, **SITE), a.iters))
            runs["torch_nms"].append(timed(lambda: torch_decide(torch_pairs(masks, idx), ranked, idx, **SITE), a.iters))
            runs["segmaps"].append(timed(lambda: MN.build_seg_maps([packed] * 4, keeps), a.iters))
            runs["end_to_end"].append(timed(end_to_end, a.iters))
        best = {k: min(v) for k, v in runs.items()}
        tiles = (N + 63) // 64
        shape = {"N": N, "H": H, "W": W, "kept": int(res.selected.shape[0])}
        lines.append({
            "variant": "hip", **shape, "ms_pack": round(best["pack"], 4), "ms_pair_counts": round(best["pairs"], 4),
            "ms_select_with_sort_and_count_readback": round(best["select"], 4),
            "ms_decide_as_select_minus_pair_counts": round(best["select"] - best["pairs"], 4),
            "ms_segment_maps_4_levels": round(best["segmaps"], 4), "ms_end_to_end": round(best["end_to_end"], 4),
            "pack_input_GBps": round(N * H * W / best["pack"] / 1e6, 1),
            "pair_word_ANDs_per_s_needed_pairs": round(N * (N + 1) / 2 * W64 / best["pairs"] * 1e3, 0),
            "pair_word_ANDs_per_s_run_tiles": round(tiles * (tiles + 1) / 2 * 4096 * W64 / best["pairs"] * 1e3, 0),
            "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items() if not k.startswith("torch")}})
        lines.append({
            "variant": "torch", **shape, "ms_float_matmul_pairs": round(best["torch_pairs"], 4),
            "ms_decide": round(best["torch_decide"], 4), "ms_pairs_and_decide": round(best["torch_nms"], 4),
            "pairs_ratio_torch_over_hip": round(best["torch_pairs"] / best["pairs"], 2),
            "pairs_and_decide_ratio_torch_over_hip_select": round(best["torch_nms"] / best["select"], 2),
            "pair_table_equal": pairs_equal, "selected_equal": bool(torch.equal(want, res.selected)),
            "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items() if k.startswith("torch")}})
        if (H, W) not in host_done:
            host_done[(H, W)] = host_pair_loop(masks[:HOST_N].cpu(), a.reference)
        per_pair, source = host_done[(H, W)]
        lines.append({"variant": "host_loop", **shape, "host_work": True, "source": source, "measured_at_N": HOST_N,
                      "ms_per_pair_measured": round(per_pair * 1e3, 4),
                      "s_all_pairs_extrapolated": round(per_pair * N * (N + 1) / 2, 2)})
        for ln in lines[-3:]:
            print(json.dumps(ln), flush=True)
        del masks, packed, inter_t, res
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(ln) for ln in lines) + "\n")


if __name__ == "__main__":
    main()
