"""Generate tests/golden/ref_codebook_init.npz by running the REFERENCE's own
ResidualVectorQuantizationWithClustering.fit_quantizers (utils/vq_utils.py:43-81:
one sklearn MiniBatchKMeans per level, residuals through torch.cdist argmin) on
the CPU, for np.random.seed(0..4), 2 levels of 64 clusters, on one seeded
(4096, 64) table.  Pins the quality of langsplatv2_amd/codebook_init.py
(tests/test_codebook_init.py): the reference's fit is unseeded, so its own
seed-to-seed spread of the residual energy is the margin the test allows.

The table: unit-normalised rows drawn from 80 random directions with unequal
weights, plus noise 0.5 / sqrt(D) (clustered, more clusters than codes, as CLIP
features of a scene are).

Stored (data only): the table, the residual energy sum |r|^2 after every level
for every seed (float64, from the reference's own forward indices), and seed
0's centres and indices.

Run:  LSR_REFERENCE=<reference checkout> python tests/golden/make_ref_codebook_init.py
(needs scikit-learn; only the resulting .npz is committed and travels)."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

if not os.environ.get("LSR_REFERENCE"):
    sys.exit("set LSR_REFERENCE to the reference checkout (the directory holding utils/vq_utils.py)")
sys.path.insert(0, os.environ["LSR_REFERENCE"])
from utils import vq_utils  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_codebook_init.npz")
M, D, K, L = 4096, 64, 64, 2
SEEDS = range(5)


def table():
    rng = np.random.RandomState(7)
    dirs = rng.standard_normal((80, D))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    w = rng.random_sample(80) ** 2 + 0.05
    lab = rng.choice(80, size=M, p=w / w.sum())
    x = dirs[lab] + 0.5 / np.sqrt(D) * rng.standard_normal((M, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x.astype(np.float32))


def main():
    x = table()
    out = {"table": x}
    energy = np.zeros((len(SEEDS), L), dtype=np.float64)
    for s in SEEDS:
        np.random.seed(s)
        rvq = vq_utils.ResidualVectorQuantizationWithClustering(L, K, D, "cpu")
        with contextlib.redirect_stdout(io.StringIO()):   # the class prints per level
            rvq.fit_quantizers(torch.from_numpy(x))
            _, idx = rvq(torch.from_numpy(x))
        r = x.astype(np.float64)
        for lv in range(L):
            r = r - rvq.quantizers[lv].numpy().astype(np.float64)[idx[lv].numpy()]
            energy[s, lv] = float((r * r).sum())
        if s == 0:
            out["centers_seed0"] = np.stack([q.numpy() for q in rvq.quantizers]).astype(np.float32)
            out["indices_seed0"] = np.stack([i.numpy() for i in idx]).astype(np.uint8)
        print("seed", s, "residual energy per level", energy[s])
    out["energy"] = energy
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
