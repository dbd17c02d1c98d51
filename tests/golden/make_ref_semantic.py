"""Generate tests/golden/ref_semantic.npz by running the REFERENCE's own
OpenCLIPNetwork.get_semantic_map (eval/openclip_encoder.py:82-94) on the quick
weight map of ref_relevancy.npz, on the CPU.

As in make_ref_relevancy.py, empty stub modules stand in for open_clip and
torchvision (neither is needed by get_semantic_map), and the method is called
unbound on a SimpleNamespace carrying the two attributes it reads
(semantic_embeds, neg_embeds).  The semantic map it is given is built by the
reference's post-render lines (eval_lerf.py:214-218) in float64 and made
contiguous (the reference's `.view(-1, c)` needs that); the stored labels are
the reference's float64 labels, and the reference's own fp32 labels are
asserted equal to them here.

Cases (C, N) = (5, 4), (13, 4), (61, 4), (252, 4): the first C rows of one
seeded label table and one set of 4 negatives, unit vectors rounded to fp16
(the dtype of the reference's CLIP embeddings) and stored as such.  In the
cases with C >= 13, label 7 is a copy of label 2 and negative 1 a copy of
label 4 (duplicate rows, and a negative equal to a label: exact ties).

Stored per case: the float64 similarities mm(sem_map[i].view(-1, c), p.T)
(L, H, W, C + N) — for (252, 4) only each pixel's two largest values
(L, H, W, 2), because the full matrix alone is 1.4 MB and a committed file
stays under 1 MiB — and the labels (L, H, W) int16.

Run:  LSR_REFERENCE=<reference tree> python tests/golden/make_ref_semantic.py
(only the .npz is committed).
"""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

REF = os.environ["LSR_REFERENCE"]
for name in ("open_clip", "torchvision"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.path.insert(0, REF)
from eval.openclip_encoder import OpenCLIPNetwork  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_semantic.npz")
CASES = [(5, 4), (13, 4), (61, 4), (252, 4)]
TOP2_ONLY = (252, 4)


def semantic_map(wmap, cb, dtype):
    """eval_lerf.py:214-218, then the (L, H, W, Df) permutation of its callers."""
    L, K, Df = cb.shape
    D, H, W = wmap.shape
    w = torch.from_numpy(wmap).to(dtype).view(L, K, H, W).view(L, K, H * W)
    c = torch.from_numpy(cb).to(dtype).permute(0, 2, 1)
    f = torch.einsum("ldk,lkn->ldn", c, w).view(L, Df, H, W)
    f = f / (f.norm(dim=1, keepdim=True) + 1e-10)
    return f.permute(0, 2, 3, 1).contiguous()


def unit16(g, n, d):
    e = g.standard_normal((n, d))
    return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float16)


def main():
    z = np.load(os.path.join(HERE, "ref_relevancy.npz"))
    wmap, cb = z["weight_map"], z["codebooks"]
    L, K, Df = cb.shape
    H, W = wmap.shape[1:]
    zy, zx = z["zero_pixel"]
    g = np.random.default_rng(20250317)
    table, negs = unit16(g, max(c for c, _ in CASES), Df), unit16(g, 4, Df)
    table_dup, negs_dup = table.copy(), negs.copy()
    table_dup[7] = table[2]
    negs_dup[1] = table[4]
    out = dict(label_table=table, label_table_dup=table_dup, neg_embeds=negs, neg_embeds_dup=negs_dup,
               cases=np.array(CASES))
    for C, N in CASES:
        dup = C >= 13
        sem = (table_dup if dup else table)[:C].astype(np.float32)
        neg = (negs_dup if dup else negs)[:N].astype(np.float32)

        def run(dtype):
            ns = SimpleNamespace(semantic_embeds=torch.from_numpy(sem), neg_embeds=torch.from_numpy(neg))
            with torch.no_grad():
                return OpenCLIPNetwork.get_semantic_map(ns, semantic_map(wmap, cb, dtype)).numpy()

        l64, l32 = run(torch.float64), run(torch.float32)
        assert l64.shape == (L, H, W) and l64.dtype == np.int64
        assert np.array_equal(l64, l32), "the reference's fp32 and float64 labels differ"
        sm = semantic_map(wmap, cb, torch.float64)
        p = torch.from_numpy(np.concatenate([sem, neg])).double()
        sims = torch.stack([torch.mm(sm[i].view(-1, Df), p.T) for i in range(L)]).view(L, H, W, C + N).numpy()
        top2 = -np.sort(-sims, axis=-1)[..., :2] if C + N > 1 else None
        margin = top2[..., 0] - top2[..., 1]
        assert np.all(l64[:, zy, zx] == 0), "the zero pixel"
        if dup:
            assert not np.any(l64 == 7), "label 7 duplicates label 2 and must never win"
        print(f"C={C} N={N}: {int((margin < 2e-6).sum())} of {margin.size} pixels with a top-2 margin < 2e-6, "
              f"-1 on {100.0 * float((l64 == -1).mean()):.0f} %")
        out[f"sims_{C}_{N}"] = top2 if (C, N) == TOP2_ONLY else sims
        out[f"labels_{C}_{N}"] = l64.astype(np.int16)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
