"""The render kernels' group tails: the ML forward blends staged candidates in
groups of 4 (a partial group waits for the next 64-entry chunk of the tile
list, the list's last group may be partial) and the backward replays them in
groups of 16.  These frames put chosen numbers of candidates into chosen 8x8
blocks, so every tail shape occurs:

  counts   per-block staged counts 1..8 (n mod 4 = 0, 1, 2, 3; lists of 1-3
           candidates), an empty tile, a candidate with opacity below 1/255,
           blocks of the tile column cut by the image's right edge;
  chunks   tiles of exactly 64, 65 and 128 instances whose blocks carry 1, 2
           and 3 candidates across the chunk boundary;
  stack    an opaque stack: pixels terminate inside a full group and inside
           the list's last, partial group.

Frames are make_case frames whose first rows are overwritten with splats at
chosen pixels (camera space = world space at yaw 0).  Small splats (sigma 0.5
px before the 0.3 px^2 dilation, opacity <= 0.5) sit within 0.75 px of a
block's centre: their cut ellipse has radius < 2.4 px, so they are staged by
that block alone.  The shapes are asserted on the oracle's outputs (CPU), with
a staging classifier that refuses to decide within a factor 1.5 of the cut."""
import functools

import numpy as np
import pytest
import torch

from harness import (GRAD_ATOL, GRAD_RTOL, assert_grad_close, make_case, oracle_problem, run_gpu_bwd_rows,
                     run_gpu_fwd_bwd)
from test_gpu_parity import _fwd_compare

W, H = 40, 36          # 3 x 3 tiles; the last tile column and row are cut by the image edge
DIMS = [16, 32]
SMALL = 0.5            # small splats' projected sigma (px), before the dilation


def _place(case, rows):
    """Overwrite the first len(rows) Gaussians: (px, py, sigma_px, opacity), depth increasing with the row."""
    g, cam = case["g"], case["cam"]
    n = len(rows)
    assert n <= g["means3D"].shape[0]
    focal = cam["W"] / (2.0 * cam["tanfovx"])
    r = np.asarray(rows, np.float64)
    z = 3.0 + 0.01 * np.arange(n)
    x = ((2 * r[:, 0] + 1) / cam["W"] - 1) * z * cam["tanfovx"]
    y = ((2 * r[:, 1] + 1) / cam["H"] - 1) * z * cam["tanfovy"]
    g["means3D"][:n] = torch.from_numpy(np.stack([x, y, z], 1)).float()
    g["scales"][:n] = torch.from_numpy(np.repeat((r[:, 2] * z / focal)[:, None], 3, 1)).float()
    g["rotations"][:n] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    g["opacities"][:n, 0] = torch.from_numpy(r[:, 3]).float()
    # everything else out of sight (behind the camera)
    g["means3D"][n:, 2] = -5.0
    return case


def _smalls(rng, block, count, opacity=None):
    """`count` small splats within 0.75 px of the centre of block (bx, by)."""
    bx, by = block
    out = []
    for _ in range(count):
        o = opacity if opacity is not None else rng.uniform(0.2, 0.5)
        out.append((bx + 3.5 + rng.uniform(-0.75, 0.75), by + 3.5 + rng.uniform(-0.75, 0.75), SMALL, o))
    return out


def _blocks_of(tile):
    tx, ty = tile
    return [(16 * tx + 8 * (s & 1), 16 * ty + 8 * (s >> 1)) for s in range(4)]


def _rows_counts(rng):
    rows = []
    for tile, counts in (((0, 0), (1, 2, 3, 4)), ((1, 0), (5, 6, 7, 8))):
        for blk, c in zip(_blocks_of(tile), counts):
            rows += _smalls(rng, blk, c)
    # tile (2, 0): its right blocks lie outside the image; block (32, 0) gets 3, one below 1/255
    rows += _smalls(rng, (32, 0), 2) + _smalls(rng, (32, 0), 1, opacity=0.003)
    # tile (2, 1), block (32, 24): one candidate; tile (2, 2) and the others stay empty
    rows += _smalls(rng, (32, 24), 1)
    rng.shuffle(rows)
    return rows


def _rows_chunks(rng):
    """Depth order = row order: a tile's first 64 rows are its first chunk."""
    def tile_rows(tile, first, second):
        blks = _blocks_of(tile)
        out = []
        for part in (first, second):
            p = [r for blk, c in zip(blks, part) for r in _smalls(rng, blk, c)]
            rng.shuffle(p)
            out += p
        return out
    rows = tile_rows((0, 0), (13, 14, 15, 22), (0, 0, 0, 0))        # 64: one chunk exactly
    rows += tile_rows((1, 0), (5, 6, 7, 46), (1, 0, 0, 0))          # 65: carries 1, 2, 3 (and 2), one entry in chunk 2
    rows += tile_rows((0, 1), (9, 10, 11, 34), (20, 20, 12, 12))    # 128: carries 1, 2, 3 into a full second chunk
    return rows


def _rows_stack(rng):
    # block (0, 0): 3 small, then 10 wide splats (sigma 5 px) of opacity 0.99 at the block's centre: the
    # centre pixels terminate at the 3rd wide splat, the corner pixels (alpha ~0.6) about 10 deep
    rows = _smalls(rng, (0, 0), 3) + [(3.5, 3.5, 5.0, 0.99)] * 10
    return rows


FRAMES = {"counts": (_rows_counts, 11), "chunks": (_rows_chunks, 12), "stack": (_rows_stack, 13)}


@functools.lru_cache(maxsize=None)
def _frame(name, D):
    """One frame, its oracle forward, upstream gradients and oracle backward: computed once, never written to."""
    from oracle import oracle as O
    build, seed = FRAMES[name]
    rows = build(np.random.default_rng(seed))
    case = _place(make_case(N=max(320, len(rows)), W=W, H=H, sh_degree=1, lang_dim=D, seed=seed), rows)
    pb = oracle_problem(case)
    ref = O.forward(pb)
    rng = np.random.default_rng(seed + 100)
    dcol = rng.standard_normal((3, H, W)).astype(np.float32)
    dlang = rng.standard_normal((D, H, W)).astype(np.float32)
    return case, pb, ref, dcol, dlang, O.backward(pb, ref, dcol, dlang)


def _staged(ref, tile, block):
    """Tile-list indices (0-based, depth order) the block stages, from the oracle's records: a candidate is
    staged when its centre lies in the block's pixel rectangle or the rectangle is well inside its cut
    ellipse, not staged when the rectangle is well outside it; anything within a factor 1.5 of the cut
    is refused (the kernel's test is conservative there, and this classifier does not restate it)."""
    gx = (W + 15) // 16
    rs, re = (int(v) for v in ref["ranges"][tile[1] * gx + tile[0]])
    bx, by = block
    out = []
    for k, gid in enumerate(ref["point_list"][rs:re]):
        x, y = (float(v) for v in ref["xy"][gid])
        ca, cb, cc, o = (float(v) for v in ref["conic_opacity"][gid])
        dx = max(bx - x, 0.0, x - (bx + 7)), max(by - y, 0.0, y - (by + 7))
        if dx == (0.0, 0.0):
            out.append(k)
            continue
        lam = np.linalg.eigvalsh(np.array([[ca, cb], [cb, cc]]))
        d2 = dx[0] ** 2 + dx[1] ** 2
        thr = 2.0 * max(np.log(255.0 * o), 0.0) + 0.05      # -2 x the exponent cut, with its margins
        far2 = (max(x - bx, bx + 7 - x)) ** 2 + (max(y - by, by + 7 - y)) ** 2
        if lam[1] * far2 * 1.5 < thr:
            out.append(k)                                    # the whole rectangle inside the cut ellipse
        else:
            assert lam[0] * d2 > 1.5 * thr, ("undecided staging", tile, block, k, lam, d2, thr)
    return out, re - rs


def _chunk_counts(staged, n):
    """The block's staged candidates per 64-entry chunk of its tile's n-entry list."""
    return [sum(1 for k in staged if k // 64 == c) for c in range((n + 63) // 64)]


# ------------------------------------------------------------- CPU: the shapes

def test_counts_frame_has_every_remainder(oracle_lib):
    ref = _frame("counts", 16)[2]
    want = {}
    for tile, counts in (((0, 0), (1, 2, 3, 4)), ((1, 0), (5, 6, 7, 8))):
        for blk, c in zip(_blocks_of(tile), counts):
            want[(tile, blk)] = c
    want[((2, 0), (32, 0))] = 3
    want[((2, 1), (32, 24))] = 1
    got = {k: len(_staged(ref, *k)[0]) for k in want}
    assert got == want
    assert {n % 4 for n in got.values()} == {0, 1, 2, 3} and {1, 2, 3} <= set(got.values())
    counts = ref["ranges"][:, 1].astype(int) - ref["ranges"][:, 0].astype(int)
    assert counts.reshape(3, 3)[2, 2] == 0 and counts.reshape(3, 3)[0, 0] == 10      # an empty tile
    assert (np.asarray(_frame("counts", 16)[0]["g"]["opacities"][:43, 0]) < 1 / 255).sum() == 1
    # the sub-1/255 candidate is staged (block (32, 0) counts 3) and contributes to no pixel
    assert counts.reshape(3, 3)[0, 2] == 3
    assert int(ref["n_contrib"][0:8, 32:40].max()) <= 3


def test_chunks_frame_has_every_carry(oracle_lib):
    ref = _frame("chunks", 16)[2]
    lens, carries = {}, {}
    for tile in ((0, 0), (1, 0), (0, 1)):
        for blk in _blocks_of(tile):
            st, n = _staged(ref, tile, blk)
            lens[tile] = n
            carries[(tile, blk)] = [c % 4 for c in _chunk_counts(st, n)[:-1]]
    assert lens == {(0, 0): 64, (1, 0): 65, (0, 1): 128}
    for tile in ((1, 0), (0, 1)):
        assert [carries[(tile, b)][0] for b in _blocks_of(tile)] == [1, 2, 3, 2]
    # the 65-entry tile: its 65th entry joins block 0's carried candidate in a 2-candidate last group
    st, n = _staged(ref, (1, 0), (16, 0))
    assert _chunk_counts(st, n) == [5, 1]


def test_stack_frame_terminates_inside_groups(oracle_lib):
    ref = _frame("stack", 16)[2]
    st, n = _staged(ref, (0, 0), (0, 0))
    assert n == 13 and st == list(range(13))            # 3 full groups + a last group of 1
    last = ref["n_contrib"][0:8, 0:8].astype(int)        # 1-based position of the last contributor
    # a pixel whose last contributor is followed by a wide opaque splat terminated at that splat (staged index = last)
    term = last[last < n]
    assert term.size > 0 and (ref["final_T"][0:8, 0:8][last < n] < 0.05).all()
    assert any(t % 4 != 0 and t < 12 for t in term), term        # inside a full group
    assert any(t == 12 for t in term), term                      # in the last, partial group
    assert (last == n).any() or (term.min() < term.max())        # pixels stop at different depths


# ------------------------------------------------------------------ GPU parity

def _grad_request():
    from langsplatv2_amd import _lib
    return _lib.LSR_GWS_GEOM | _lib.LSR_GWS_LANG


@pytest.mark.gpu
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", list(FRAMES))
def test_forward_bit_exact(gpu, oracle_lib, name, D):
    """Colour, language, final_T, n_contrib and radii bit for bit, for the inference forward and for the
    forward of a call with a pending backward (the list-writing instantiation)."""
    case = _frame(name, D)[0]
    _fwd_compare(case, gpu, oracle_lib)
    ref, got = _fwd_compare(case, gpu, oracle_lib, grad_request=_grad_request())
    assert got["has_grad_ws"] and got["has_lists"]


@pytest.mark.gpu
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", list(FRAMES))
def test_gradients_close(gpu, oracle_lib, name, D):
    case, pb, ref, dcol, dlang, rb = _frame(name, D)
    got = run_gpu_fwd_bwd(case, gpu, dcol, dlang)
    np.testing.assert_array_equal(got["color"], ref["color"])
    np.testing.assert_array_equal(got["lang"], ref["lang"])
    np.testing.assert_array_equal(got["radii"], ref["radii"])
    pairs = dict(means3D="dmeans3D", shs="dsh", scales="dscales", rotations="drot", opacities="dopacity",
                 language_feature_precomp="dlang", means2D="dmean2D")
    for k, r in pairs.items():
        print(name, D, k, assert_grad_close(k, got["grad_" + k], rb[r], GRAD_RTOL, GRAD_ATOL))


@pytest.mark.gpu
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", list(FRAMES))
def test_deterministic_backward_repeats(gpu, oracle_lib, name, D):
    case, pb, ref, dcol, dlang, rb = _frame(name, D)
    a = run_gpu_bwd_rows(case, gpu, dcol, dlang, deterministic=True)
    b = run_gpu_bwd_rows(case, gpu, dcol, dlang, deterministic=True)
    assert a["has_lists"] and a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert float(np.abs(a["rows"]).max()) > 1e-3
