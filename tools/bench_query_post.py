"""Post-process of the relevancy maps on one MI355X: the fused path
(langsplatv2_amd.segment.segment_maps + localize_maps, csrc/query_post.hip)
against the torch code a caller ran before it.

Every caller of get_max_across_quick in the reference walks the (L, Q, H, W)
maps plane by plane: a 29 x 29 AvgPool2d, a blend, a min-max normalisation, a
threshold, a 7 x 7 AvgPool2d majority, IoU sums and a level arg-max
(eval_lerf.py:111-156), then a second pass of 29 x 29 pools with .max() and
torch.nonzero for the localisation (eval_lerf.py:158-200).  `torch_segment` and
`torch_localize` below restate those two loops in torch, with the reference's
host round trips (.tolist(), .item(), nonzero, a CPU score vector) where it has
them; the segmentation loop blends its input in place, so it gets a fresh copy
of the maps per call, as get_max_across_quick hands the reference a new tensor.

Synthetic maps: L = 3 levels x Q = 4 prompts of smooth relevancy-like fields in
(0, 1) plus white noise, one rectangular annotation mask and box per prompt.
Timed, all in one process and alternating, `--repeats` times `--iters` calls
each, every window closed by a device synchronise.  Prints one JSON line per
resolution (medians, repeat-to-repeat spread, the byte model of the fused path
and the share of the measured copy rate it reaches, and how far the two paths'
results agree) and, with --out, writes the lines to that file.

  python tools/bench_query_post.py [--iters 20] [--repeats 5] [--out profiles/query_post_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from langsplatv2_amd import segment  # noqa: E402

HBM_PEAK = 8.0e12        # B/s, datasheet
HBM_MEASURED = 6.29e12   # B/s, float4 copy (the rate DESIGN.md sets k_quick_query against)


def torch_segment(valid_map, thresh, gt_masks):
    """eval_lerf.py:111-156 restated; valid_map (L, Q, H, W) is blended in place."""
    n_head, n_prompt, h, w = valid_map.shape
    dev = valid_map.device
    chosen_iou, chosen_lvl, masks = [], [], []
    for k in range(n_prompt):
        iou_lvl = torch.zeros(n_head, device=dev)
        mask_lvl = torch.zeros((n_head, h, w), device=dev)
        for i in range(n_head):
            pool = torch.nn.AvgPool2d(kernel_size=29, stride=1, padding=14, count_include_pad=False).to(dev)
            filtered = pool(valid_map[i][k].unsqueeze(0).unsqueeze(0))
            valid_map[i][k] = 0.5 * (filtered.squeeze(0).squeeze(0) + valid_map[i][k])
            out = valid_map[i][k]
            out = out - torch.min(out)
            out = out / (torch.max(out) + 1e-9)
            out = torch.clip(out * 2.0 - 1.0, 0, 1)
            pred = (out > thresh).type(torch.uint8)
            pool7 = torch.nn.AvgPool2d(kernel_size=7, stride=1, padding=3, count_include_pad=False).to(dev)
            pred = (pool7(pred.float().unsqueeze(0).unsqueeze(0)) > 0.5).type(torch.uint8).squeeze(0).squeeze(0)
            mask_lvl[i] = pred
            inter = torch.sum(torch.logical_and(gt_masks[k], pred))
            union = torch.sum(torch.logical_or(gt_masks[k], pred))
            iou_lvl[i] = inter / union
        iou_lvl.tolist()
        score_lvl = torch.zeros((n_head,), device=dev)
        for i in range(n_head):
            score_lvl[i] = valid_map[i, k].max()
        lvl = torch.argmax(score_lvl)
        chosen_iou.append(iou_lvl[lvl].cpu().numpy().item())
        chosen_lvl.append(lvl.cpu().numpy().item())
        masks.append(mask_lvl)
    return chosen_iou, chosen_lvl, masks


def torch_localize(valid_map, boxes):
    """eval_lerf.py:158-200 restated; boxes[k]: (n, 4) x1 y1 x2 y2 on the host."""
    n_head, n_prompt, h, w = valid_map.shape
    dev = valid_map.device
    acc, points = 0, []
    for k in range(n_prompt):
        pool = torch.nn.AvgPool2d(kernel_size=29, stride=1, padding=14, count_include_pad=False).to(dev)
        filtered = pool(valid_map[:, k].unsqueeze(1)).squeeze(1)
        score_lvl = torch.zeros((n_head,))
        coord_lvl = []
        for i in range(n_head):
            score = filtered[i].max()
            coord_lvl.append(torch.nonzero((filtered[i] == score).type(torch.uint8)))
            score_lvl[i] = score
        head = torch.argmax(score_lvl)
        coords = coord_lvl[head]
        points.append(coords[0].tolist())
        hit = False
        for x1, y1, x2, y2 in boxes[k].reshape(-1, 4).tolist():
            for c in coords:
                if min(x1, x2) <= c[1] <= max(x1, x2) and min(y1, y2) <= c[0] <= max(y1, y2):
                    hit = True
                    break
            if hit:
                break
        acc += int(hit)
    return acc, points


def make_maps(L, Q, H, W, dev):
    gen = torch.Generator().manual_seed(H * 10000 + W)
    z = torch.randn(L * Q, 1, H // 8 + 2, W // 8 + 2, generator=gen).to(dev)
    z = torch.nn.functional.interpolate(z, size=(H, W), mode="bicubic", align_corners=False)
    z = torch.nn.functional.avg_pool2d(z, 31, stride=1, padding=15)
    z = 3.0 * z / z.std(dim=(-2, -1), keepdim=True)
    v = 0.96 * torch.sigmoid(z) + 0.02 + 0.02 * (torch.rand(z.shape, generator=gen).to(dev) - 0.5)
    return v.view(L, Q, H, W).contiguous()


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
    ap.add_argument("--sizes", default="1280x800,1920x1080")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_query_post.py needs a ROCm GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    L, Q, thresh = 3, 4, 0.4
    lines = []
    for W, H in (tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")):
        rel = make_maps(L, Q, H, W, dev)
        gt = torch.zeros(Q, H, W, dtype=torch.uint8, device=dev)
        boxes = []
        for q in range(Q):
            y, x = divmod(int(rel[0, q].argmax()), W)
            y0, y1, x0, x1 = max(0, y - H // 6), min(H - 1, y + H // 6), max(0, x - W // 6), min(W - 1, x + W // 6)
            gt[q, y0:y1 + 1, x0:x1 + 1] = 1
            boxes.append(torch.tensor([[x0, y0, x1, y1]], dtype=torch.float64))

        fns = {
            "segment": lambda: segment.segment_maps(rel, thresh, gt_masks=gt),
            "localize": lambda: segment.localize_maps(rel),
            "fused": lambda: (segment.segment_maps(rel, thresh, gt_masks=gt), segment.localize_maps(rel)),
            "torch_segment": lambda: torch_segment(rel.clone(), thresh, gt),
            "torch_localize": lambda: torch_localize(rel, boxes),
            "torch": lambda: (torch_segment(rel.clone(), thresh, gt), torch_localize(rel, boxes)),
            "clone": lambda: rel.clone(),
        }
        slow = {"torch_segment", "torch_localize", "torch"}
        # the two paths on the same maps: masks of the chosen levels, levels, IoUs, localisation
        keep = rel.clone()
        s, loc = fns["fused"]()
        (t_iou, t_lvl, t_masks), (t_acc, t_pts) = fns["torch"]()
        assert torch.equal(rel, keep), "the fused path must not write its input"
        q_idx = torch.arange(Q, device=dev)
        agree = {
            "levels_equal": s.level.tolist() == t_lvl,
            "mask_pixels_differing": int(sum((s.masks[:, q] != t_masks[q].to(torch.uint8)).sum() for q in range(Q))),
            "max_abs_iou_diff": max(abs(a - b) for a, b in zip(s.iou[s.level, q_idx].tolist(), t_iou)),
            "localisation_points_equal": loc.yx_chosen.tolist() == t_pts,
            "hits_equal": segment.hits(loc, boxes) == t_acc,
        }
        for fn in fns.values():   # warm-up of every shape timed below
            fn()
            fn()
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                ms[k].append(window(fn, max(3, args.iters // 4) if k in slow else args.iters))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        px = L * Q * H * W
        # smooth (segment): 4 read + 4 blend written; mask: 4 blend + 1 annotation read, 1 written;
        # smooth (localize): 4 read, nothing written
        model = {"segment": px * (4 + 4 + 4 + 1 + 1), "localize": px * 4}
        model["fused"] = model["segment"] + model["localize"]
        bps = {k: model[k] / (med[k] * 1e-3) for k in model}
        lines.append(json.dumps({
            "workload": f"relevancy post-process (29x29 box blend, threshold {thresh}, 7x7 majority, IoU, level, "
                        f"localisation), L={L} levels x Q={Q} prompts, {W}x{H}, synthetic maps",
            "iters": args.iters, "repeats": args.repeats,
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_spread": {k: round(v, 4) for k, v in spread.items()},
            "torch_over_fused": round(med["torch"] / med["fused"], 1),
            "fused_faster_than_torch_beyond_spread":
                max(ms["fused"]) + spread["fused"] + spread["torch"] < min(ms["torch"]),
            "byte_model": model,
            "GBps_of_byte_model": {k: round(v / 1e9, 1) for k, v in bps.items()},
            "share_of_6.29TBps_measured_copy": {k: round(v / HBM_MEASURED, 3) for k, v in bps.items()},
            "share_of_8.0TBps_spec": {k: round(v / HBM_PEAK, 3) for k, v in bps.items()},
            "agreement_with_torch": agree}))
        print(lines[-1], flush=True)
        del rel, gt
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
