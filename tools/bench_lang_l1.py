"""Feature-phase loss with --l1_loss at one training view: forward + backward
of language_feature_loss(l1=True) with fused_l1 on (lsr_lang_l1_forward /
_backward, plus the fused cosine kernel where --cos_loss is set) and off (the
torch formulation over the Df-wide map, train.py:151-167), on the same GPU.
Synthetic seeded inputs: K = 64 codes, Df = 512, S segments in coherent
regions, a tenth of the pixels masked.

  python tools/bench_lang_l1.py [--iters 10 --S 200 --out profiles/lang_l1_bench.json]
Shapes 960x540, 1280x800 and 1920x1080; --l1_loss, --l1_loss --normalize and
--cos_loss --l1_loss --normalize.  Prints one JSON line per measurement (ms per
fwd+bwd over --iters iterations of either path, peak allocated bytes beyond the
inputs) and writes them all to --out.

  LSR_LIB=<liblsr.so> python tools/bench_lang_l1.py --split NAME [--out profiles/lang_l1_ab.json]
times the forward and the backward of language_l1_loss separately at 1080p
(median of --iters) for the library LSR_LIB points at and stores the row under
NAME in --out, next to the rows already there: the A/B of a build variant
(`make -C langsplatv2_amd/csrc variant NAME=ch8 VFLAGS=-DL1_CH=8`).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from langsplatv2_amd.lang_loss import language_feature_loss, language_l1_loss  # noqa: E402

SHAPES = [(540, 960), (800, 1280), (1080, 1920)]
CONFIGS = {"l1": dict(normalize=False, cos=False), "l1+normalize": dict(normalize=True, cos=False),
           "cos+l1+normalize": dict(normalize=True, cos=True)}


def measure(fn, iters, dev):
    for _ in range(2):
        fn()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / iters * 1e3, torch.cuda.max_memory_allocated(dev) - base


def inputs(H, W, S, dev, K=64, Df=512):
    g = torch.Generator(device=dev).manual_seed(0)
    wm = torch.softmax(2 * torch.randn(K, H, W, device=dev, generator=g), 0).requires_grad_(True)
    cb = torch.randn(1, K, Df, device=dev, generator=g).requires_grad_(True)
    feat = torch.nn.functional.normalize(torch.randn(S, Df, device=dev, generator=g), dim=1)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    seg = (((yy // 60) * 37 + (xx // 80)) % S).to(torch.int32)
    seg[torch.rand(H, W, device=dev, generator=g) < 0.1] = -1
    return wm, cb, seg, feat


def split(a, dev):
    """Forward and backward of language_l1_loss at 1080p, separately, for the loaded library."""
    H, W = SHAPES[-1]
    wm, cb, seg, feat = inputs(H, W, a.S, dev)
    row = {"H": H, "W": W, "S": a.S, "Df": 512, "iters": a.iters}
    for normalize in (False, True):
        fw, bw = [], []
        for i in range(a.iters + 2):
            wm.grad = cb.grad = None
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            loss = language_l1_loss(wm, cb, seg, feat, normalize=normalize)
            e[1].record()
            loss.backward()
            e[2].record()
            torch.cuda.synchronize(dev)
            if i >= 2:
                fw.append(e[0].elapsed_time(e[1]))
                bw.append(e[1].elapsed_time(e[2]))
        key = "l1+normalize" if normalize else "l1"
        row[key] = {"fwd_ms": round(sorted(fw)[len(fw) // 2], 3), "bwd_ms": round(sorted(bw)[len(bw) // 2], 3)}
    print(json.dumps({a.split: row}), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "lang_l1_ab.json")
    rows = json.load(open(out)) if os.path.exists(out) else {}
    rows[a.split] = row
    with open(out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=200)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--split", metavar="NAME", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.split:
        return split(a, dev)
    a.out = a.out or os.path.join(ROOT, "profiles", "lang_l1_bench.json")
    K, Df, S = 64, 512, a.S
    rows = []
    for H, W in SHAPES:
        wm, cb, seg, feat = inputs(H, W, S, dev)
        for name, flags in CONFIGS.items():
            def step(fused):
                wm.grad = cb.grad = None
                language_feature_loss(wm, cb, seg, feat, l1=True, fused_l1=fused, **flags).backward()
            ms_f, peak_f = measure(lambda: step(True), a.iters, dev)
            wm.grad = cb.grad = None
            torch.cuda.empty_cache()
            ms_t, peak_t = measure(lambda: step(False), a.iters, dev)
            wm.grad = cb.grad = None
            torch.cuda.empty_cache()
            with torch.no_grad():
                l_f = float(language_feature_loss(wm, cb, seg, feat, l1=True, fused_l1=True, **flags))
                l_t = float(language_feature_loss(wm, cb, seg, feat, l1=True, **flags))
            row = {"H": H, "W": W, "S": S, "Df": Df, "config": name, "fused_ms_fwd_bwd": round(ms_f, 4),
                   "torch_ms_fwd_bwd": round(ms_t, 4), "speedup_fused": round(ms_t / ms_f, 2),
                   "fused_peak_bytes": peak_f, "torch_peak_bytes": peak_t, "loss_fused": l_f, "loss_torch": l_t}
            rows.append(row)
            print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev), "iters": a.iters, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
