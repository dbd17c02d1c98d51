"""Binning with exact per-tile key counts, and two more binning shapes.

The one-wave tile sort sizes its network by the tile's key count: ceil(n / 64)
keys per lane, every count up to 4 and the even counts above.  The first frame
puts a chosen number of keys into every tile, so every keys-per-lane count,
both sides of every 64-key boundary and the 1024 / 1025 class boundary are
hit, with equal depths in every tile (the id breaks the tie), 28 count chunks
that all have instances in the same tiles, a tile count (56) that is no
multiple of 64 or 4, and empty tiles.  A second frame of the same construction
puts the upper sort classes at their exact boundaries (BIG_TARGETS).  The other
two are a two-band frame and a single-tile frame.  All against the oracle: radii, ranges, point_list,
n_contrib, images (the checks of test_gpu_parity's forward comparison).  Runs
on the GPU box."""
import numpy as np
import pytest
import torch

from harness import assert_img, fwd_atol, make_case, oracle_problem, run_gpu_forward
from langsplatv2_amd.scenes import make_camera

pytestmark = pytest.mark.gpu

W, H, GX, GY = 128, 112, 8, 7
# keys per tile: 1, 2, both sides of every 64-key boundary up to 1024, a tile in
# the middle of a keys-per-lane step and one of the first 4-wave class
TARGETS = [1, 2] + [64 * r + d for r in range(1, 17) for d in (-1, 0, 1)] + [600, 1500]
# both sides of every class boundary above 1024 (2048, 4096: the 4-wave block
# sorts; 8192: the chunked sort), a chunked-sort tile of three 4096-key chunks
# and one of five, whose last merge stage spans 32768 slots
BIG_TARGETS = [2048, 2049, 4096, 4097, 8192, 8193, 12000, 16385]


def exact_count_case(seed=0, targets=TARGETS):
    """Tile t holds exactly n_t Gaussians, all projected to its centre pixel
    (7.5, 7.5) and far smaller than a tile; in each tile the first n/8 depths
    repeat the next n/8 (the id breaks the tie); the tiles past the targets
    stay empty (four with TARGETS)."""
    rng = np.random.default_rng(seed)
    cam = make_camera(W, H, yaw_deg=0.0)
    tiles = rng.permutation(GX * GY)
    counts = np.zeros(GX * GY, dtype=np.int64)
    counts[tiles[:len(targets)]] = targets
    xs, ys, zs = [], [], []
    for t in range(GX * GY):
        n = int(counts[t])
        if n == 0:
            continue
        z = rng.uniform(2.0, 12.0, n).astype(np.float32)
        d = n // 8
        z[:d] = z[d:2 * d]
        cx, cy = 16 * (t % GX) + 7.5, 16 * (t // GX) + 7.5
        xs.append(z * np.float32(cam["tanfovx"] * ((2 * cx + 1) / W - 1)))
        ys.append(z * np.float32(cam["tanfovy"] * ((2 * cy + 1) / H - 1)))
        zs.append(z)
    means = np.stack([np.concatenate(xs), np.concatenate(ys), np.concatenate(zs)], 1).astype(np.float32)
    means = means[rng.permutation(means.shape[0])]
    N = means.shape[0]
    rot = np.zeros((N, 4), dtype=np.float32)
    rot[:, 0] = 1.0
    g = dict(means3D=torch.from_numpy(means), scales=torch.full((N, 3), 1e-4), rotations=torch.from_numpy(rot),
             opacities=torch.full((N, 1), 0.5), colors_precomp=torch.from_numpy(rng.random((N, 3), dtype=np.float32)),
             sh_degree=0)
    return dict(cam=cam, g=g, bg=(0.0, 0.0, 0.0), scale_modifier=1.0, quick=False), counts


def assert_forward(case, ref, got):
    np.testing.assert_array_equal(got["radii"], ref["radii"])
    np.testing.assert_array_equal(got["tiles_touched"], ref["tiles_touched"].astype(np.int32))
    assert got["num_rendered"] == ref["num_rendered"]
    np.testing.assert_array_equal(got["ranges"], ref["ranges"].astype(np.int32))
    np.testing.assert_array_equal(got["point_list"], ref["point_list"].astype(np.int32))
    np.testing.assert_array_equal(got["n_contrib"], ref["n_contrib"].astype(np.int32))
    fa = fwd_atol(case)
    assert_img(got["final_T"], ref["final_T"], fa, "final_T")
    assert_img(got["color"], ref["color"], fa, "color")
    assert_img(got["lang"], ref["lang"], fa, "lang")


def test_exact_tile_counts(gpu, oracle_lib):
    case, counts = exact_count_case()
    N = case["g"]["means3D"].shape[0]
    assert N == 28215 == sum(TARGETS)
    ref = oracle_lib.forward(oracle_problem(case))
    # the frame is what it claims: every Gaussian one instance, every tile its target
    assert ref["num_rendered"] == N
    rr = np.asarray(ref["ranges"]).reshape(GX * GY, 2).astype(np.int64)
    np.testing.assert_array_equal(rr[:, 1] - rr[:, 0], counts)
    assert int((counts == 0).sum()) == 4
    got = run_gpu_forward(case, gpu)
    assert_forward(case, ref, got)
    # the in-bucket order before the sort is free to vary from launch to launch; the sorted lists must not
    again = run_gpu_forward(case, gpu)
    np.testing.assert_array_equal(again["point_list"], got["point_list"])
    np.testing.assert_array_equal(again["ranges"], got["ranges"])


def test_exact_tile_counts_upper_classes(gpu, oracle_lib):
    """The classes above the one-wave sort at their exact boundaries: 2048 / 2049
    and 4096 / 4097 (k_tile_sort_blk<8> | <16> | <32>), 8192 / 8193 (the last block
    sort | k_tile_sort_big), and chunked sorts of three and of five chunks."""
    case, counts = exact_count_case(seed=1, targets=BIG_TARGETS)
    N = case["g"]["means3D"].shape[0]
    assert N == 57060 == sum(BIG_TARGETS)
    ref = oracle_lib.forward(oracle_problem(case))
    assert ref["num_rendered"] == 57060
    rr = np.asarray(ref["ranges"]).reshape(GX * GY, 2).astype(np.int64)
    np.testing.assert_array_equal(rr[:, 1] - rr[:, 0], counts)
    assert int((counts == 0).sum()) == 48
    got = run_gpu_forward(case, gpu)
    assert_forward(case, ref, got)
    again = run_gpu_forward(case, gpu)
    np.testing.assert_array_equal(again["point_list"], got["point_list"])
    np.testing.assert_array_equal(again["ranges"], got["ranges"])


# two bands (70 tile rows > the 68 of one band) of two tile columns; one tile for everything
SHAPES = {
    "two_bands_32x1120": dict(N=5000, W=32, H=1120, sh_degree=None, seed=21),
    "single_tile_16x16": dict(N=3000, W=16, H=16, sh_degree=None, seed=22),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_binning_shapes(name, gpu, oracle_lib):
    case = make_case(**SHAPES[name])
    ref = oracle_lib.forward(oracle_problem(case))
    got = run_gpu_forward(case, gpu)
    assert_forward(case, ref, got)
