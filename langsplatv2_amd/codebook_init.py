"""k-means codebook initialisation of the feature phase, on the GPU.

The reference starts its feature phase (train.py:78-85) with

    features = load_2d_language_feature(dataset.lf_path, device)
    rvq = ResidualVectorQuantizationWithClustering(levels, 64, 512, device)      utils/vq_utils.py:43-104
    rvq.fit_quantizers(features)
    codebooks = torch.stack(rvq.quantizers, dim=0)

where fit_quantizers pulls the (M, 512) table to the host, runs an unseeded
sklearn MiniBatchKMeans per level and re-uploads everything for an M x K
torch.cdist.  Here the nearest-centre search and the per-cluster means are HIP
kernels (csrc/kmeans.hip, C ABI lsr_kmeans_*): the search on the exact-f32
MFMA with ties to the lowest index, the means without float atomics, so the
same seed and inputs give bit-identical codebooks.  `fit_codebooks` seeds every
level with greedy k-means++ and runs full-table Lloyd iterations;
`ResidualVectorQuantizationWithClustering` has the reference class's surface,
so `from langsplatv2_amd.codebook_init import ResidualVectorQuantizationWithClustering`
replaces `from utils.vq_utils import ResidualVectorQuantizationWithClustering`.
There is no CPU path.
"""
from __future__ import annotations

import math

import torch

from . import _lib

MAX_CLUSTERS = 256
MAX_DIM = 1024
DEFAULT_INIT_SIZE = 65536


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _shape(M, K, D, who):
    if not 1 <= K <= MAX_CLUSTERS:
        raise ValueError(f"{who}: {K} centres (the kernels take 1..{MAX_CLUSTERS})")
    if D % 4 != 0 or not 4 <= D <= MAX_DIM:
        raise ValueError(f"{who}: feature dim {D} (the kernels take a multiple of 4 in 4..{MAX_DIM})")
    if M >= 2 ** 31:
        raise ValueError(f"{who}: {M} rows (the kernels take fewer than 2^31)")


def _table(x, who, name="x"):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{who}: {name} must be a 2-D tensor (rows, dim), got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    return x


def _device(who, **tensors):
    for n, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {n} must be a ROCm device tensor (there is no CPU path)")


def _args(x, centers, who):
    _table(x, who)
    _table(centers, who, "centers")
    if x.shape[1] != centers.shape[1]:
        raise ValueError(f"{who}: x {tuple(x.shape)} and centers {tuple(centers.shape)} differ in feature dim")
    _shape(x.shape[0], centers.shape[0], x.shape[1], who)
    _device(who, x=x, centers=centers)
    return x.detach().contiguous().float(), centers.detach().to(x.device).contiguous().float()


class _Lloyd:
    """The workspace of one (M, K, D) problem and the three kernel calls on it."""

    def __init__(self, M, K, D, device):
        self.M, self.K, self.D, self.device = M, K, D, device
        self.lib = _lib.load()
        nbytes = self.lib.lsr_kmeans_workspace_bytes(M, K, D)
        if nbytes == 0:
            raise ValueError(f"k-means: shape (M={M}, K={K}, D={D}) is not supported")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)

    def prepare(self, centers):
        _lib.check(self.lib.lsr_kmeans_prepare(centers.data_ptr(), self.K, self.D, self.ws.data_ptr(),
                                               _stream(self.device)), "lsr_kmeans_prepare")

    def assign(self, x, residual=False):
        a = torch.empty(self.M, dtype=torch.int32, device=self.device)
        d = torch.empty(self.M, dtype=torch.float32, device=self.device)
        r = torch.empty_like(x) if residual else None
        _lib.check(self.lib.lsr_kmeans_assign(x.data_ptr(), self.M, self.D, self.K, self.ws.data_ptr(), a.data_ptr(),
                                              d.data_ptr(), r.data_ptr() if residual else None,
                                              _stream(self.device)), "lsr_kmeans_assign")
        return a, d, r

    def update(self, x, a):
        """(K, D) means and (K,) int32 counts; the new centres are prepared for the next assign."""
        c = torch.empty((self.K, self.D), dtype=torch.float32, device=self.device)
        n = torch.empty(self.K, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.lsr_kmeans_update(x.data_ptr(), a.data_ptr(), self.M, self.D, self.K, self.ws.data_ptr(),
                                              c.data_ptr(), n.data_ptr(), _stream(self.device)), "lsr_kmeans_update")
        return c, n


def assign_codes(x: torch.Tensor, centers: torch.Tensor, return_dist: bool = False):
    """Index (int64, (M,)) of the nearest of the (K, D) centres for every row of the
    (M, D) table x, ties to the lowest index; with return_dist also the squared
    distance (fp32, >= 0).  What torch.cdist(x, centers).argmin(dim=1) gives
    (utils/vq_utils.py:77-78), without the M x K matrix."""
    x, centers = _args(x, centers, "assign_codes")
    M, D = x.shape
    if M == 0:
        idx = torch.empty(0, dtype=torch.int64, device=x.device)
        return (idx, torch.empty(0, dtype=torch.float32, device=x.device)) if return_dist else idx
    km = _Lloyd(M, centers.shape[0], D, x.device)
    km.prepare(centers)
    a, d, _ = km.assign(x)
    return (a.long(), d) if return_dist else a.long()


def kmeans_step(x: torch.Tensor, centers: torch.Tensor):
    """One Lloyd iteration: (new_centers (K, D), counts (K,) int64, inertia 0-d fp64).
    Rows go to their nearest centre, every centre moves to the mean of its rows;
    a centre without rows stays and has count 0.  inertia is the sum of the
    squared distances to the old centres.  Bit-identical from run to run."""
    x, centers = _args(x, centers, "kmeans_step")
    M, D = x.shape
    K = centers.shape[0]
    if M == 0:
        return (centers.clone(), torch.zeros(K, dtype=torch.int64, device=x.device),
                torch.zeros((), dtype=torch.float64, device=x.device))
    km = _Lloyd(M, K, D, x.device)
    km.prepare(centers)
    a, d, _ = km.assign(x)
    c, n = km.update(x, a)
    return c, n.long(), d.double().sum()


def update_centers(x: torch.Tensor, assign: torch.Tensor, centers: torch.Tensor):
    """The update half of a Lloyd iteration for a given assignment ((M,) integer
    indices into the (K, D) centers): (new_centers, counts (K,) int64).  A centre
    without rows stays and has count 0."""
    x, centers = _args(x, centers, "update_centers")
    M, D = x.shape
    K = centers.shape[0]
    if assign.dim() != 1 or assign.shape[0] != M:
        raise ValueError(f"update_centers: assign {tuple(assign.shape)} for {M} rows")
    _device("update_centers", assign=assign)
    if M == 0:
        return centers.clone(), torch.zeros(K, dtype=torch.int64, device=x.device)
    km = _Lloyd(M, K, D, x.device)
    km.prepare(centers)
    c, n = km.update(x, assign.detach().to(torch.int32).contiguous())
    return c, n.long()


def relocate_empty(assign: torch.Tensor, dist: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """Every cluster with count 0 takes over one of the rows farthest from their
    centres: E empty clusters take the E rows of largest dist, both in ascending
    index order, by rewriting `assign` in place (the next update then puts the
    centre on that row).  Returns the rows taken."""
    empty = torch.nonzero(counts == 0).flatten()
    E = int(empty.numel())
    if E == 0:
        return empty
    far = torch.sort(dist, descending=True, stable=True).indices[:E].sort().values
    assign[far] = empty[:far.numel()].to(assign.dtype)
    return far


def _levels(codebooks, who):
    levels = list(codebooks.unbind(0)) if isinstance(codebooks, torch.Tensor) and codebooks.dim() == 3 else codebooks
    if isinstance(levels, torch.Tensor) or len(levels) == 0:
        raise ValueError(f"{who}: codebooks must be an (L, K, D) tensor or a list of (K, D) tensors")
    return list(levels)


def quantize(features: torch.Tensor, codebooks):
    """Residual quantisation of the (M, D) features by the levels of `codebooks`
    ((L, K, D) or a list of (K, D)): (quantized_sum (M, D), [indices (M,) int64
    per level]), the reference class's forward (utils/vq_utils.py:83-104)."""
    levels = _levels(codebooks, "quantize")
    _table(features, "quantize", "features")
    residual, total, indices = None, None, []
    for li, c in enumerate(levels):
        x, c = _args(features if residual is None else residual, c, "quantize")
        M, D = x.shape
        if M == 0:
            indices.append(torch.empty(0, dtype=torch.int64, device=x.device))
            total = torch.zeros_like(x)
            continue
        km = _Lloyd(M, c.shape[0], D, x.device)
        km.prepare(c)
        a, _, residual = km.assign(x, residual=li + 1 < len(levels))
        idx = a.long()
        indices.append(idx)
        q = c[idx]
        total = q if total is None else total + q
        if residual is None:
            residual = x
    return total, indices


def _seed_centers(S, K, gen):
    """Greedy k-means++ on the (n, D) sample S: every step draws 2 + floor(ln K)
    candidates with probability proportional to the squared distance to the
    nearest centre so far and keeps the one that lowers the potential most."""
    n = S.shape[0]
    dev = S.device
    n_local = 2 + int(math.log(K))
    centers = torch.empty((K, S.shape[1]), dtype=torch.float32, device=dev)
    first = torch.randint(n, (1,), generator=gen, device=dev)
    centers[0] = S[first[0]]
    closest = (S - centers[0]).square().sum(1)
    for k in range(1, K):
        cum = closest.double().cumsum(0)
        r = torch.rand(n_local, generator=gen, device=dev, dtype=torch.float64) * cum[-1]
        cand = torch.searchsorted(cum, r).clamp_(max=n - 1)
        dc = torch.stack([(S - S[cand[j]]).square().sum(1) for j in range(n_local)])
        dc = torch.minimum(dc, closest[None])
        best = dc.double().sum(1).argmin()
        closest = dc[best]
        centers[k] = S[cand[best]]
    return centers


def fit_codebooks(features: torch.Tensor, num_levels: int, num_clusters: int, seed: int = 0, max_iter: int = 30,
                  tol: float = 1e-4, init_size: int | None = None, return_history: bool = False):
    """Residual k-means codebooks (num_levels, num_clusters, D) fp32 of the (M, D)
    feature table: per level greedy k-means++ on a seeded subsample of
    `init_size` rows (default: all rows up to 65,536), then full-table Lloyd
    iterations until the inertia drops by less than `tol` relative or `max_iter`
    is reached, with every empty cluster moved to the farthest row before each
    update; the level's residual x - c[assign] is the next level's table.  The
    same seed and inputs give bit-identical codebooks.  With return_history also
    the inertia of every assign, a list per level."""
    _table(features, "fit_codebooks", "features")
    M, D = features.shape
    K, L = int(num_clusters), int(num_levels)
    if L < 1:
        raise ValueError(f"fit_codebooks: num_levels={num_levels}")
    _shape(M, K, D, "fit_codebooks")
    if M < K:
        raise ValueError(f"fit_codebooks: {M} rows for {K} clusters")
    if max_iter < 1:
        raise ValueError(f"fit_codebooks: max_iter={max_iter}")
    _device("fit_codebooks", features=features)
    x = features.detach().contiguous().float()
    dev = x.device
    n_init = min(M, DEFAULT_INIT_SIZE if init_size is None else max(int(init_size), K))
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    km = _Lloyd(M, K, D, dev)
    books, history = [], []
    for level in range(L):
        if n_init < M:
            S = x[torch.randperm(M, generator=gen, device=dev)[:n_init].sort().values]
        else:
            S = x
        centers = _seed_centers(S, K, gen)
        del S
        km.prepare(centers)
        hist, prev = [], None
        for _ in range(max_iter):
            a, d, _r = km.assign(x)
            inertia = float(d.double().sum())
            hist.append(inertia)
            if prev is not None and prev - inertia < tol * prev:
                break   # the centres are the ones this assign used
            prev = inertia
            relocate_empty(a, d, torch.bincount(a, minlength=K))
            centers, _n = km.update(x, a)
        books.append(centers)
        history.append(hist)
        if level + 1 < L:
            x = km.assign(x, residual=True)[2]
    out = torch.stack(books, 0)
    return (out, history) if return_history else out


class ResidualVectorQuantizationWithClustering(torch.nn.Module):
    """Drop-in for the reference class (utils/vq_utils.py:43-104): fit_quantizers
    fills `.quantizers` with one (num_clusters, feature_dim) fp32 device tensor per
    level, forward returns (quantized, [indices per level]).  Seeded: the same
    seed and features give the same quantizers."""

    def __init__(self, num_levels, num_clusters, feature_dim, device, seed=0):
        super().__init__()
        self.num_levels = num_levels
        self.num_clusters = num_clusters
        self.feature_dim = feature_dim
        self.device = device
        self.seed = seed
        self.quantizers = []

    def fit_quantizers(self, features):
        _table(features, "fit_quantizers", "features")
        if features.shape[1] != self.feature_dim:
            raise ValueError(f"fit_quantizers: features {tuple(features.shape)}, feature_dim={self.feature_dim}")
        books = fit_codebooks(features.to(self.device), self.num_levels, self.num_clusters, seed=self.seed)
        self.quantizers.extend(books.unbind(0))

    def forward(self, features):
        return quantize(features, self.quantizers)


__all__ = ["assign_codes", "kmeans_step", "update_centers", "quantize", "fit_codebooks", "relocate_empty",
           "ResidualVectorQuantizationWithClustering"]
