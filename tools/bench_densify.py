"""densify_and_prune at N = 1M, SH degree 3 (about 10 % of the rows cloned, 5 % split,
5 % pruned): the fused plan + apply (langsplatv2_amd.densify.densify_tensors, including its
host read-back and output allocation) vs the reference's torch op sequence
(densify_and_prune_torch) on the same GPU and inputs, and the apply kernel alone against its
byte floor (bytes it must move / the 6.29 TB/s streaming-copy rate of the MI355X).

  python tools/bench_densify.py [--n 1000000] [--iters 20] [--out profiles/densify_bench.json]
Times are device events after warm-up, variants alternated, best of three rounds.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from langsplatv2_amd import _lib  # noqa: E402
from langsplatv2_amd.densify import GROUPS, densify_and_prune_torch, densify_tensors  # noqa: E402

COPY_TBPS = 6.29   # measured float4 copy, MI355X
KNOBS = dict(max_grad=0.0002, min_opacity=0.005, extent=4.0, percent_dense=0.01)


def inputs(n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.rand(*s, device=dev, generator=g)   # noqa: E731
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    u = r(n)
    sel = u < 0.15                                    # 15 % reach max_grad ...
    large = u < 0.05                                  # ... a third of them are large: split
    ms = torch.where(large, 0.1, 0.02) * (0.5 + 0.5 * r(n))
    params = {"xyz": rn(n, 3), "f_dc": rn(n, 1, 3), "f_rest": 0.1 * rn(n, 15, 3),
              "opacity": torch.where(r(n, 1) < 0.05, -6.0, 1.0) + 0.1 * rn(n, 1),
              "scaling": torch.log(ms)[:, None] + torch.log(0.3 + 0.7 * r(n, 3)), "rotation": rn(n, 4)}
    # one component carries ms itself, so no row sits at the 0.04 / 0.4 thresholds (fused and torch must agree)
    params["scaling"][torch.arange(n, device=dev), (r(n) * 3).long().clamp(max=2)] = torch.log(ms)
    params = {k: v.float().contiguous() for k, v in params.items()}
    moments = {k: (0.01 * rn(*v.shape), 0.001 * r(*v.shape)) for k, v in params.items()}
    accum = torch.where(sel, 0.001, 0.00005).reshape(n, 1) * 3.0
    denom = torch.full((n, 1), 3.0, device=dev)
    return params, moments, accum, denom, torch.zeros(n, device=dev), rn(n, 2, 3)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    params, moments, accum, denom, radii, noise = inputs(a.n, dev)
    kw = dict(max_screen_size=20, noise=noise, **KNOBS)
    fused = lambda: densify_tensors(params, moments, accum, denom, radii, **kw)   # noqa: E731
    torch_seq = lambda: densify_and_prune_torch(params, moments, accum, denom, radii, **kw)   # noqa: E731
    fp, fm, _, res = fused()
    tp, tm, _, tres = torch_seq()
    assert res == tres, (res, tres)
    same = all(torch.equal(fp[k], tp[k]) for k in ("f_dc", "f_rest", "opacity", "rotation")) and \
        all(torch.equal(fm[k][0], tm[k][0]) for k in GROUPS)

    # the apply kernel alone, on a plan made once
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty(lib.lsr_densify_workspace_bytes(a.n), dtype=torch.uint8, device=dev)
    counts = (ctypes.c_int64 * 6)()
    plan = lambda: _lib.check(lib.lsr_densify_plan(   # noqa: E731
        a.n, accum.data_ptr(), denom.data_ptr(), params["scaling"].data_ptr(), params["opacity"].data_ptr(),
        KNOBS["max_grad"], KNOBS["percent_dense"] * KNOBS["extent"], KNOBS["min_opacity"], 1, 0.1 * KNOBS["extent"],
        ws.data_ptr(), counts, stream), "lsr_densify_plan")
    plan()
    n_out = sum(counts[:4])
    assert n_out == res.n_after
    src, dst = (ctypes.c_void_p * 18)(), (ctypes.c_void_p * 18)()
    for g, k in enumerate(GROUPS):
        for part, (s, d) in enumerate(((params[k], fp[k]), (moments[k][0], fm[k][0]), (moments[k][1], fm[k][1]))):
            src[6 * part + g], dst[6 * part + g] = s.data_ptr(), d.data_ptr()
    apply = lambda: _lib.check(lib.lsr_densify_apply(a.n, n_out, ws.data_ptr(), 45, src, dst, noise.data_ptr(),   # noqa: E731
                                                     stream), "lsr_densify_apply")
    # bytes the gather must move: every output element written, every parameter element read, the moments
    # read for the copied rows only, one map word per row
    row = 59
    moved = 4 * (n_out * 3 * row + n_out * row + counts[0] * 2 * row + n_out)
    floor_ms = moved / (COPY_TBPS * 1e12) * 1e3

    ms = {"fused": [], "torch": [], "plan": [], "apply": []}
    for _ in range(3):   # alternate, so a busy neighbour hits every variant alike
        ms["fused"].append(timed(fused, a.iters))
        ms["torch"].append(timed(torch_seq, a.iters))
        ms["plan"].append(timed(plan, a.iters))
        ms["apply"].append(timed(apply, a.iters))
    best = {k: min(v) for k, v in ms.items()}
    line = {"N": a.n, "sh_degree": 3, "n_after": res.n_after, "n_clone": res.n_clone, "n_split": res.n_split,
            "n_pruned": res.n_pruned, "copied_fields_equal_torch": bool(same),
            "ms_fused_plan_apply": round(best["fused"], 4), "ms_torch_sequence": round(best["torch"], 4),
            "speedup_fused": round(best["torch"] / best["fused"], 2),
            "ms_plan": round(best["plan"], 4), "ms_apply_kernel": round(best["apply"], 4),
            "apply_bytes": int(moved), "apply_floor_ms": round(floor_ms, 4),
            "apply_TBps": round(moved / best["apply"] / 1e9, 3), "apply_over_floor": round(best["apply"] / floor_ms, 2),
            "ms_runs": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
