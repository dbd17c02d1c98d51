"""langsplatv2_amd/codebook_init.py: the k-means codebook initialisation of the
feature phase (csrc/kmeans.hip, C ABI lsr_kmeans_*), replacing
ResidualVectorQuantizationWithClustering.fit_quantizers / forward
(utils/vq_utils.py:43-104, train.py:78-85).

The checker is a float64 restatement in this file.  The bounds (DESIGN §4,
"k-means assign and update"), with u = 2^-24 and gamma_n = n u / (1 - n u):

  assign   a score |c|^2 - 2 x.c carries D + 1 roundings, so it is within
           e(x, c) = gamma_{D+2} (sum c_d^2 + 2 sum |x_d c_d|) of its exact value,
           and the chosen centre a satisfies
               d64(x, c_a) <= min_k d64(x, c_k) + e(x, c_a) + e(x, c_kmin);
  dist     within e(x, c_a) + gamma_D sum x_d^2 of d64(x, c_a), and >= 0;
  update   a mean of n rows is within gamma_n sum |x_d| / n of the float64 mean
           (n - 1 additions in a fixed order, one division).

Quality is pinned against the reference's own fit (tests/golden/ref_codebook_init.npz,
made by tests/golden/make_ref_codebook_init.py): the residual energy after every
level must be <= ref_max + (ref_max - ref_min) over the reference's five seeds.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from langsplatv2_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_codebook_init.npz")
U = 2.0 ** -24
# (M, D, K): one k-step and one column block; the two sides of a 64-row tile; D = 512;
# K padded to 64; the largest K with a partial last tile and more tiles than waves
CASES = [(1, 4, 16), (63, 64, 64), (65, 64, 64), (257, 512, 64), (1000, 128, 48), (4099, 512, 256)]


def gamma(n):
    return n * U / (1.0 - n * U)


@functools.lru_cache(maxsize=None)
def case(M, D, K):
    """Seeded rows and centres (centres: rows plus noise, so clusters are populated and
    near misses exist); shared, never modified."""
    g = torch.Generator().manual_seed(1000 * M + 10 * D + K)
    x = torch.randn(M, D, generator=g)
    c = x[torch.randint(M, (K,), generator=g)] + 0.3 * torch.randn(K, D, generator=g)
    return x.contiguous(), c.contiguous()


def d64(x, c):
    return torch.cdist(x.double(), c.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2


def score_err(x, c, idx):
    """e(x_i, c_idx[i]) per row, float64."""
    x, cc = x.double(), c.double()[idx]
    return gamma(x.shape[1] + 2) * ((cc * cc).sum(1) + 2.0 * (x * cc).abs().sum(1))


def check_nearest(x, c, idx, dist=None, what=""):
    """The assign bound (and the dist bound) for every row; idx, dist on the CPU."""
    M, D = x.shape
    dm = d64(x, c)
    rows = torch.arange(M)
    assert idx.dtype == torch.int64 and idx.shape == (M,)
    assert int(idx.min()) >= 0 and int(idx.max()) < c.shape[0], what
    da = dm[rows, idx]
    dmin, kmin = dm.min(1)
    ea = score_err(x, c, idx)
    slack = dmin + ea + score_err(x, c, kmin) - da
    print(f"{what}: worst assign slack {float(slack.min()):.3e} (>= 0 passes)")
    assert bool((slack >= 0).all()), (what, float(slack.min()))
    if dist is not None:
        assert dist.dtype == torch.float32 and bool((dist >= 0).all()), what
        err = (dist.double() - da).abs()
        bound = ea + gamma(D) * (x.double() ** 2).sum(1)
        print(f"{what}: worst dist error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (what, float((err / bound).max()))


# ------------------------------------------------------------------- CPU ---
def test_c_abi_argument_checks():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P = ctypes.cast(buf, ctypes.c_void_p).value & ~15 or 16   # a 16-B aligned stand-in address, never dereferenced
    OK, EINVAL = 0, 1
    wsb = lib.lsr_kmeans_workspace_bytes
    assert wsb(1000, 64, 512) > 0 and wsb(0, 1, 4) > 0 and wsb((1 << 31) - 1, 256, 1024) > 0
    for args in [(10, 0, 512), (10, 257, 512), (10, 64, 6), (10, 64, 1028), (10, 64, 0), (-1, 64, 512),
                 (1 << 31, 64, 512)]:
        assert wsb(*args) == 0, args
    prep = lib.lsr_kmeans_prepare   # (centers, K, D, workspace, stream)
    for args in [(None, 64, 512, P, None), (P, 64, 512, None, None), (P, 0, 512, P, None), (P, 257, 512, P, None),
                 (P, 64, 6, P, None), (P, 64, 1028, P, None), (P + 4, 64, 512, P, None)]:
        assert prep(*args) == EINVAL, args
    asg = lib.lsr_kmeans_assign     # (x, M, D, K, workspace, assign, dist, residual_out, stream)
    for args, want in [
            ((None, 10, 512, 64, P, P, P, None, None), EINVAL),
            ((P, 10, 512, 64, None, P, P, None, None), EINVAL),
            ((P, 10, 512, 64, P, None, P, None, None), EINVAL),
            ((P, 10, 512, 64, P, P, None, None, None), EINVAL),
            ((P, 10, 512, 64, P, P, P, P, None), EINVAL),          # the residual may not alias x
            ((P + 4, 10, 512, 64, P, P, P, None, None), EINVAL),   # not 16-B aligned
            ((P, 10, 512, 0, P, P, P, None, None), EINVAL),
            ((P, 10, 512, 257, P, P, P, None, None), EINVAL),
            ((P, 10, 6, 64, P, P, P, None, None), EINVAL),
            ((P, 10, 1028, 64, P, P, P, None, None), EINVAL),
            ((P, -1, 512, 64, P, P, P, None, None), EINVAL),
            ((P, 1 << 31, 512, 64, P, P, P, None, None), EINVAL),
            ((None, 0, 512, 257, None, None, None, None, None), EINVAL),   # the shape before the no-op
            ((None, 0, 512, 64, None, None, None, None, None), OK),
    ]:
        assert asg(*args) == want, (args, want)
    upd = lib.lsr_kmeans_update     # (x, assign, M, D, K, workspace, centers_out, counts_out, stream)
    for args, want in [
            ((None, P, 10, 512, 64, P, P, P, None), EINVAL),
            ((P, None, 10, 512, 64, P, P, P, None), EINVAL),
            ((P, P, 10, 512, 64, None, P, P, None), EINVAL),
            ((P, P, 10, 512, 64, P, None, P, None), EINVAL),
            ((P, P, 10, 512, 64, P, P, None, None), EINVAL),
            ((P, P, 10, 512, 0, P, P, P, None), EINVAL),
            ((P, P, 10, 512, 257, P, P, P, None), EINVAL),
            ((P, P, 10, 6, 64, P, P, P, None), EINVAL),
            ((P, P, 10, 1028, 64, P, P, P, None), EINVAL),
            ((P, P, -1, 512, 64, P, P, P, None), EINVAL),
            ((None, None, 0, 6, 64, None, None, None, None), EINVAL),      # the shape before the no-op
            ((None, None, 0, 512, 64, None, None, None, None), OK),
    ]:
        assert upd(*args) == want, (args, want)


def test_python_argument_checks():
    import langsplatv2_amd
    from langsplatv2_amd import codebook_init as CI
    x, c = torch.rand(10, 8), torch.rand(4, 8)
    for fn in (CI.assign_codes, CI.kmeans_step):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            fn(x, c)
        with pytest.raises(ValueError, match="2-D"):
            fn(torch.rand(8), c)
        with pytest.raises(ValueError, match="2-D"):
            fn(x, torch.rand(1, 4, 8))
        with pytest.raises(ValueError, match="feature dim"):
            fn(x, torch.rand(4, 12))
        with pytest.raises(ValueError, match="257 centres"):
            fn(x, torch.rand(257, 8))
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(torch.rand(10, 6), torch.rand(4, 6))
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(torch.rand(10, 1028), torch.rand(4, 1028))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        CI.quantize(x, torch.rand(2, 4, 8))
    with pytest.raises(ValueError, match="codebooks"):
        CI.quantize(x, c)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        CI.fit_codebooks(x, 1, 4)
    with pytest.raises(ValueError, match="10 rows for 16 clusters"):
        CI.fit_codebooks(x, 1, 16)
    with pytest.raises(ValueError, match="num_levels"):
        CI.fit_codebooks(x, 0, 4)
    with pytest.raises(ValueError, match="300 centres"):
        CI.fit_codebooks(torch.rand(400, 8), 1, 300)
    with pytest.raises(ValueError, match="multiple of 4"):
        CI.fit_codebooks(torch.rand(10, 6), 1, 4)
    rvq = CI.ResidualVectorQuantizationWithClustering(2, 4, 8, "cpu")
    assert rvq.quantizers == [] and (rvq.num_levels, rvq.num_clusters, rvq.feature_dim) == (2, 4, 8)
    with pytest.raises(ValueError, match="feature_dim"):
        rvq.fit_quantizers(torch.rand(10, 12))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        rvq.fit_quantizers(x)
    for name in ("assign_codes", "kmeans_step", "quantize", "fit_codebooks",
                 "ResidualVectorQuantizationWithClustering"):
        assert getattr(langsplatv2_amd, name) is getattr(CI, name)


def test_fixture_is_data_only():
    z = np.load(GOLD)
    assert sorted(z.files) == ["centers_seed0", "energy", "indices_seed0", "table"]
    assert z["table"].shape == (4096, 64) and z["table"].dtype == np.float32
    assert z["energy"].shape == (5, 2) and z["centers_seed0"].shape == (2, 64, 64)
    assert os.path.getsize(GOLD) < (1 << 20)


# ------------------------------------------------------------------- GPU ---
@pytest.mark.gpu
@pytest.mark.parametrize("shape", CASES)
def test_assign_is_a_nearest_centre_within_the_bound(gpu, shape):
    from langsplatv2_amd.codebook_init import assign_codes
    x, c = case(*shape)
    idx, dist = assign_codes(x.to(gpu), c.to(gpu), return_dist=True)
    check_nearest(x, c, idx.cpu(), dist.cpu(), f"assign {shape}")
    assert torch.equal(assign_codes(x.to(gpu), c.to(gpu)), idx)


@pytest.mark.gpu
def test_ties_go_to_the_lowest_index(gpu):
    from langsplatv2_amd.codebook_init import assign_codes
    g = torch.Generator().manual_seed(5)
    c = torch.randn(64, 64, generator=g)
    c[40] = c[3]   # bitwise-identical centres
    near = c[3] + 0.01 * torch.randn(150, 64, generator=g)
    x = torch.cat([near, torch.randn(150, 64, generator=g)])
    idx = assign_codes(x.to(gpu), c.to(gpu)).cpu()
    assert bool((idx[:150] == 3).all()) and not bool((idx == 40).any())
    # x = 0 against +e0 / -e0: equal scores, the lower index, in either order
    e0 = torch.zeros(2, 4)
    e0[0, 0], e0[1, 0] = 1.0, -1.0
    z = torch.zeros(17, 4)
    assert bool((assign_codes(z.to(gpu), e0.to(gpu)) == 0).all())
    assert bool((assign_codes(z.to(gpu), e0.flip(0).contiguous().to(gpu)) == 0).all())


@pytest.mark.gpu
def test_a_row_equal_to_a_centre_is_assigned_to_it(gpu):
    from langsplatv2_amd.codebook_init import assign_codes
    c = torch.randn(48, 128, generator=torch.Generator().manual_seed(6))
    idx, dist = assign_codes(c.to(gpu), c.to(gpu), return_dist=True)
    idx, dist = idx.cpu(), dist.cpu()
    assert torch.equal(idx, torch.arange(48))
    bound = score_err(c, c, idx) + gamma(128) * (c.double() ** 2).sum(1)
    assert bool((dist >= 0).all()) and bool((dist.double() <= bound).all())


@pytest.mark.gpu
def test_empty_table(gpu):
    from langsplatv2_amd import codebook_init as CI
    x, c = torch.empty(0, 64, device=gpu), torch.randn(16, 64, device=gpu)
    idx, dist = CI.assign_codes(x, c, return_dist=True)
    assert idx.shape == (0,) and idx.dtype == torch.int64 and dist.shape == (0,) and dist.dtype == torch.float32
    new, counts, inertia = CI.kmeans_step(x, c)
    assert torch.equal(new, c) and int(counts.sum()) == 0 and float(inertia) == 0.0
    total, ids = CI.quantize(x, c[None])
    assert total.shape == (0, 64) and len(ids) == 1 and ids[0].shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CASES)
def test_update_counts_and_means(gpu, shape):
    from langsplatv2_amd.codebook_init import assign_codes, kmeans_step
    x, c = case(*shape)
    M, D, K = shape
    idx = assign_codes(x.to(gpu), c.to(gpu)).cpu()
    new, counts, inertia = kmeans_step(x.to(gpu), c.to(gpu))
    new, counts = new.cpu(), counts.cpu()
    assert new.dtype == torch.float32 and new.shape == (K, D) and counts.dtype == torch.int64
    ref_counts = torch.bincount(idx, minlength=K)
    assert torch.equal(counts, ref_counts)
    sums = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, x.double())
    asum = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, x.double().abs())
    worst = 0.0
    for k in range(K):
        n = int(ref_counts[k])
        if n == 0:
            assert torch.equal(new[k], c[k]), k   # an empty cluster keeps its centre
            continue
        err = (new[k].double() - sums[k] / n).abs()
        bound = gamma(n) * asum[k] / n
        assert bool((err <= bound).all()), (shape, k, n, float(err.max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"update {shape}: worst mean error / bound {worst:.3f}")
    # the inertia is the float64 sum of the fp32 dist values: within the sum of their bounds
    ref_inertia = float(d64(x, c)[torch.arange(M), idx].sum())
    slack = float((score_err(x, c, idx) + gamma(D) * (x.double() ** 2).sum(1)).sum())
    assert abs(float(inertia) - ref_inertia) <= slack * (1.0 + 1e-9)


@pytest.mark.gpu
def test_empty_cluster_moves_to_the_farthest_row(gpu):
    from langsplatv2_amd import codebook_init as CI
    g = torch.Generator().manual_seed(8)
    x = torch.randn(300, 64, generator=g)
    x[17] = 0.0
    x[17, 5] = 40.0                       # the one row far from every centre: the largest dist is unique
    c = x[:30].clone()                    # centres on rows 0..29,
    c[17] = x[200]                        # but none on the far row
    c[9] = 1.0e3                          # far outside the data: no row is nearest to it
    xd, cd = x.to(gpu), c.to(gpu)
    new, counts, _ = CI.kmeans_step(xd, cd)
    assert int(counts[9]) == 0 and torch.equal(new[9].cpu(), c[9])
    idx, dist = CI.assign_codes(xd, cd, return_dist=True)
    assert int(dist.argmax()) == 17
    a = idx.clone()
    far = CI.relocate_empty(a, dist, torch.bincount(idx, minlength=30))
    assert far.tolist() == [17] and int(a[17]) == 9 and int((a != idx).sum()) == 1
    moved, counts2 = CI.update_centers(xd, a, cd)
    assert int(counts2[9]) == 1 and torch.equal(moved[9].cpu(), x[17])
    # two empties take the two largest, both in ascending index order
    d2 = torch.tensor([0.5, 9.0, 0.1, 7.0, 0.2], device=gpu)
    a2 = torch.tensor([0, 0, 2, 2, 0], dtype=torch.int32, device=gpu)
    far2 = CI.relocate_empty(a2, d2, torch.bincount(a2, minlength=4))
    assert far2.tolist() == [1, 3] and a2.tolist() == [0, 1, 2, 3, 0]


@functools.lru_cache(maxsize=None)
def _fit(seed):
    """fit_codebooks on a clustered (3000, 64) table, 2 levels of 32: (codebooks, history), on the CPU."""
    from langsplatv2_amd.codebook_init import fit_codebooks
    g = torch.Generator().manual_seed(9)
    x = torch.randn(40, 64, generator=g)[torch.randint(40, (3000,), generator=g)] + \
        0.2 * torch.randn(3000, 64, generator=g)
    cb, hist = fit_codebooks(x.to("cuda:0"), 2, 32, seed=seed, init_size=1024, return_history=True)
    return cb.cpu(), hist


@pytest.mark.gpu
def test_bit_reproducible(gpu):
    from langsplatv2_amd.codebook_init import fit_codebooks, kmeans_step
    x, c = case(4099, 512, 256)
    a, b = kmeans_step(x.to(gpu), c.to(gpu)), kmeans_step(x.to(gpu), c.to(gpu))
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    cb0, hist0 = _fit(3)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(40, 64, generator=g)[torch.randint(40, (3000,), generator=g)] + \
        0.2 * torch.randn(3000, 64, generator=g)
    again, hist1 = fit_codebooks(x.to(gpu), 2, 32, seed=3, init_size=1024, return_history=True)
    assert again.shape == (2, 32, 64) and again.dtype == torch.float32 and again.is_cuda
    assert torch.equal(again.cpu(), cb0) and hist0 == hist1
    assert not torch.equal(_fit(4)[0], cb0)


@pytest.mark.gpu
def test_lloyd_inertia_never_rises(gpu):
    for seed in (3, 4):
        _, hist = _fit(seed)
        assert len(hist) == 2
        for lv in hist:
            assert 2 <= len(lv) <= 31
            for before, after in zip(lv, lv[1:]):
                assert after <= before * (1.0 + 1e-6), (seed, before, after)


@pytest.mark.gpu
def test_quantize_and_the_drop_in_class(gpu):
    from langsplatv2_amd.codebook_init import ResidualVectorQuantizationWithClustering, quantize
    from langsplatv2_amd.train_loop import LanguageState
    g = torch.Generator().manual_seed(10)
    M, D, K, L = 777, 512, 64, 3
    x = torch.randn(M, D, generator=g)
    cbs = torch.stack([torch.randn(K, D, generator=g) * s for s in (1.0, 0.6, 0.4)])
    total, ids = quantize(x.to(gpu), cbs.to(gpu))
    assert len(ids) == L and total.shape == (M, D) and total.dtype == torch.float32
    # vq_utils.py:83-104 level by level on this pipeline's fp32 residuals, distances in float64
    r, want = x, None
    for lv in range(L):
        idx = ids[lv].cpu()
        check_nearest(r, cbs[lv], idx, None, f"quantize level {lv}")
        q = cbs[lv][idx]
        want = q if want is None else want + q
        r = r - q
    assert torch.equal(total.cpu(), want)
    # a list of levels is taken as well
    total2, ids2 = quantize(x.to(gpu), [c.to(gpu) for c in cbs])
    assert torch.equal(total2, total) and all(torch.equal(p, q) for p, q in zip(ids, ids2))
    rvq = ResidualVectorQuantizationWithClustering(1, K, D, gpu, seed=0)
    assert isinstance(rvq, torch.nn.Module)
    rvq.fit_quantizers(x.to(gpu))
    assert isinstance(rvq.quantizers, list) and len(rvq.quantizers) == 1
    for qz in rvq.quantizers:
        assert qz.shape == (K, D) and qz.dtype == torch.float32 and qz.device == gpu
    codebooks = torch.stack(rvq.quantizers, dim=0)   # train.py:83
    out, oids = rvq(x.to(gpu))
    t3, i3 = quantize(x.to(gpu), codebooks)
    assert torch.equal(out, t3) and torch.equal(oids[0], i3[0])
    N = 10
    ls = LanguageState(torch.zeros(N, 3, device=gpu), torch.zeros(N, 16, 3, device=gpu), torch.zeros(N, 1, device=gpu),
                       torch.zeros(N, 3, device=gpu), torch.zeros(N, 4, device=gpu), torch.zeros(N, K, device=gpu),
                       codebooks)
    assert torch.equal(ls.codebooks.detach(), codebooks)


def _energies(x, cb, ids):
    r, out = x.double(), []
    for lv in range(cb.shape[0]):
        r = r - cb[lv].double()[ids[lv]]
        out.append(float((r * r).sum()))
    return out


@pytest.mark.gpu
def test_quality_against_the_reference_fit(gpu):
    """sum |r|^2 after level 0 / level 1.  The reference's five seeds span 927.6 .. 982.1 /
    739.1 .. 756.5, so the bounds are 1036.6 / 773.9; measured on an MI355X for seeds 0, 1, 2:
    931.0 / 722.3, 932.0 / 728.1, 913.5 / 719.6."""
    from langsplatv2_amd.codebook_init import fit_codebooks, quantize
    z = np.load(GOLD)
    x = torch.from_numpy(z["table"])
    hi, lo = z["energy"].max(0), z["energy"].min(0)
    bound = hi + (hi - lo)
    for seed in (0, 1, 2):
        cb = fit_codebooks(x.to(gpu), 2, 64, seed=seed)
        _, ids = quantize(x.to(gpu), cb)
        en = _energies(x, cb.cpu(), [i.cpu() for i in ids])
        print(f"seed {seed}: residual energy {en[0]:.1f} / {en[1]:.1f} (bound {bound[0]:.1f} / {bound[1]:.1f})")
        for lv in range(2):
            assert en[lv] <= bound[lv], (seed, lv, en[lv], bound[lv])


@pytest.mark.gpu
def test_quantize_with_the_reference_centres(gpu):
    from langsplatv2_amd.codebook_init import quantize
    z = np.load(GOLD)
    x, cb = torch.from_numpy(z["table"]), torch.from_numpy(z["centers_seed0"])
    ref_ids = torch.from_numpy(z["indices_seed0"].astype(np.int64))
    _, ids = quantize(x.to(gpu), cb.to(gpu))
    r = x
    rows = torch.arange(x.shape[0])
    for lv in range(2):
        idx = ids[lv].cpu()
        check_nearest(r, cb[lv], idx, None, f"reference centres level {lv}")
        dm = d64(r, cb[lv])
        slack = dm[rows, ref_ids[lv]] + score_err(r, cb[lv], idx) + score_err(r, cb[lv], ref_ids[lv]) - dm[rows, idx]
        assert bool((slack >= 0).all()), (lv, float(slack.min()))
        print(f"level {lv}: {int((idx == ref_ids[lv]).sum())} of {len(idx)} indices equal the reference's")
        r = r - cb[lv][idx]
