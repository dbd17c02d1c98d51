"""Feature-phase codebook initialisation at M = 262,144 rows of 512 dims, K = 64,
one level: the HIP Lloyd iteration (langsplatv2_amd.codebook_init) vs the
reference's formulation on the same GPU (utils/vq_utils.py:77-78 torch.cdist +
argmin, the means by index_add_), on a seeded clustered table.

  python tools/bench_codebook_init.py [--iters 20] [--out profiles/codebook_init_bench.json]
      [--reference <reference checkout>]   (with scikit-learn: also the reference class's own
                                            fit_quantizers wall time, which is host work)
Prints one JSON line per variant (ms per Lloyd iteration: assign, update; ms of the whole fit).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from langsplatv2_amd import codebook_init as CI  # noqa: E402

M, D, K = 262144, 512, 64
# per row and iteration: assign reads the row (4 D) and writes index + dist (8 B); update reads the row and its index
ASSIGN_BYTES_PER_ROW = 4 * D + 8
UPDATE_BYTES_PER_ROW = 4 * D + 4


def table(dev):
    """Unit rows around 200 random directions with unequal weights, noise 0.5 / sqrt(D)."""
    g = torch.Generator(device=dev).manual_seed(0)
    dirs = torch.nn.functional.normalize(torch.randn(200, D, device=dev, generator=g), dim=1)
    w = torch.rand(200, device=dev, generator=g) ** 2 + 0.05
    lab = torch.multinomial(w, M, replacement=True, generator=g)
    x = dirs[lab] + 0.5 / D ** 0.5 * torch.randn(M, D, device=dev, generator=g)
    return torch.nn.functional.normalize(x, dim=1).contiguous()


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def torch_assign(x, c):
    return torch.cdist(x, c, p=2).argmin(dim=1)


def torch_update(x, idx, c):
    n = torch.bincount(idx, minlength=K)
    s = torch.zeros_like(c).index_add_(0, idx, x)
    return torch.where(n[:, None] > 0, s / n.clamp_min(1)[:, None], c), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", default=os.environ.get("LSR_REFERENCE"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x = table(dev)
    c = x[torch.randperm(M, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:K]].contiguous()
    km = CI._Lloyd(M, K, D, dev)
    km.prepare(c)
    idx32 = km.assign(x)[0]
    idx64 = idx32.long()
    # alternate the variants so a busy neighbour hits both alike
    runs = {"hip_assign": [], "hip_assign_residual": [], "hip_update": [], "torch_assign": [], "torch_update": []}
    for _ in range(3):
        runs["hip_assign"].append(timed(lambda: km.assign(x), a.iters))
        runs["torch_assign"].append(timed(lambda: torch_assign(x, c), a.iters))
        runs["hip_assign_residual"].append(timed(lambda: km.assign(x, residual=True), a.iters))
        runs["hip_update"].append(timed(lambda: km.update(x, idx32), a.iters))
        km.prepare(c)
        runs["torch_update"].append(timed(lambda: torch_update(x, idx64, c), a.iters))
    best = {k: min(v) for k, v in runs.items()}
    agree = float((torch_assign(x, c) == idx64).float().mean())
    lines = [
        {"variant": "hip_lloyd_iteration", "M": M, "D": D, "K": K, "ms_assign": round(best["hip_assign"], 4),
         "ms_assign_with_residual": round(best["hip_assign_residual"], 4), "ms_update": round(best["hip_update"], 4),
         "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items() if k.startswith("hip")},
         "assign_GBps": round(ASSIGN_BYTES_PER_ROW * M / best["hip_assign"] / 1e6, 1),
         "assign_TFLOPs": round(2.0 * M * D * K / best["hip_assign"] / 1e9, 2),
         "update_GBps": round(UPDATE_BYTES_PER_ROW * M / best["hip_update"] / 1e6, 1)},
        {"variant": "torch_cdist_argmin_index_add", "M": M, "D": D, "K": K, "ms_assign": round(best["torch_assign"], 4),
         "ms_update": round(best["torch_update"], 4),
         "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items() if k.startswith("torch")},
         "iteration_ratio_torch_over_hip": round((best["torch_assign"] + best["torch_update"]) /
                                                 (best["hip_assign"] + best["hip_update"]), 2),
         "indices_equal_fraction": agree},
    ]
    fits = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cb, hist = CI.fit_codebooks(x, 1, K, seed=0, return_history=True)
        torch.cuda.synchronize()
        fits.append((time.perf_counter() - t0) * 1e3)
    lines.append({"variant": "hip_fit_codebooks", "M": M, "D": D, "K": K, "levels": 1, "ms_fit": round(min(fits), 1),
                  "ms_runs": [round(t, 1) for t in fits], "lloyd_iterations": len(hist[0]),
                  "inertia_first": hist[0][0], "inertia_last": hist[0][-1]})
    try:
        import sklearn
        from sklearn.cluster import MiniBatchKMeans
        t0 = time.perf_counter()
        if a.reference:   # the reference class itself
            sys.path.insert(0, a.reference)
            from utils import vq_utils
            rvq = vq_utils.ResidualVectorQuantizationWithClustering(1, K, D, dev)
            with contextlib.redirect_stdout(io.StringIO()):
                rvq.fit_quantizers(x)
            q = rvq.quantizers[0]
        else:             # its steps restated (utils/vq_utils.py:57-68): host copy, unseeded fit, upload, cdist
            host = x.cpu().numpy()
            q = torch.tensor(MiniBatchKMeans(n_clusters=K).fit(host).cluster_centers_, device=dev, dtype=torch.float32)
            resid = torch.tensor(host, device=dev) - q[torch.cdist(torch.tensor(host, device=dev), q).argmin(dim=1)]
            del resid
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        inertia = float(CI.assign_codes(x, q, return_dist=True)[1].double().sum())
        lines.append({"variant": "reference_fit_quantizers", "host_work": True,
                      "source": "reference class" if a.reference else "restated steps", "ms_fit": round(ms, 1),
                      "inertia_last": inertia, "sklearn": sklearn.__version__})
    except ImportError as e:
        lines.append({"variant": "reference_fit_quantizers", "skipped": str(e)})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(ln) for ln in lines) + "\n")


if __name__ == "__main__":
    main()
