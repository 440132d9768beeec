"""The set-up passes of the two sorts (csrc/binning.hip) on the smallest shapes at which they can go wrong.

The depth sort's scatter kernel zeroes its per-wave u16 cursor table and turns the counts into offsets eight bins (16 bytes) at a
time, on packed halves (its third pass shares the helpers); the tile sort's scatter kernel pads its cursor rows to eight tiles,
zeroes them 16 bytes at a time, takes four tiles per access and scans the tile counts four rounds per barrier; the chunk scans
split a workgroup into tiles x segments by a compile-time pair (32 x 32 for the depth sort, 64 x 16 for the tile sorts).  None of it may change a bit: the instance list, the tile keys and the ranges are compared with the
oracle's 64-bit (tile | depth) key sort (tests/gpu_util.py: compare_forward_state).  Every case first asserts, from the oracle's own
outputs, the property of the scene that it relies on."""
import numpy as np
import pytest
import torch

from riggs_amd.rasterizer import saved_views
from tests import gpu_util as U

pytestmark = pytest.mark.gpu


def _compare(act, cam, so_out=None):
    out_o, so = so_out if so_out is not None else U.oracle_forward(act, cam, [0, 0, 0])
    color, radii, depth, alpha, s = U.hip_forward(act, cam, [0, 0, 0])
    U.compare_forward_state(so, saved_views(s), out_o, color, depth, alpha, radii)
    return so, s


def wall_scene(n_planes, N=2049 + 300, H=64, W=64):
    """Gaussians in `n_planes` planes perpendicular to the view axis of an axis-aligned camera (azimuth = elevation = 0: the
    rotation part of the view matrix holds exact zeros and ones), plane by index modulo n_planes."""
    sc, act, cam = U.activated_scene(N, 8, 43, H, W, scale=0.03, azimuth_deg=0.0, elevation_deg=0.0)
    z = np.array([0.25, -0.5], np.float32)[np.arange(N) % n_planes]
    act["means3D"][:, 2] = torch.from_numpy(z)
    return act, cam


def covering_scene(N, H=64, W=64):
    """Gaussians so large that each covers every tile of the image."""
    sc, act, cam = U.activated_scene(N, 8, 44, H, W, scale=2.0)
    return act, cam


# ---- all keys equal: every element of a wave lands in ONE bin of both digits — a u16 counter next to seven zero neighbours
# reaches 64 x STEPS, a chunk's 2048 — and the order must be the index order; then two digit values
@pytest.mark.parametrize("n_planes", [1, 2])
def test_wall_at_constant_depth(n_planes):
    act, cam = wall_scene(n_planes)
    out_o, so = U.oracle_forward(act, cam, [0, 0, 0])
    vis = so.radii > 0
    assert int(vis.sum()) > 2048 + 64, int(vis.sum())  # (more than a chunk of the depth sort)
    bits = so.depths[vis].view(np.uint32)
    assert len(np.unique(bits)) == n_planes, np.unique(bits)
    if n_planes == 1:
        # equal keys: inside every tile's list the Gaussians stand in index order
        tile = (so.keys >> np.uint64(32)).astype(np.int64)
        pl = so.point_list.astype(np.int64)
        same = tile[1:] == tile[:-1]
        assert bool((pl[1:][same] > pl[:-1][same]).all())
    so, s = _compare(act, cam, (out_o, so))
    assert int(s.counters[2]) == 0


# ---- one tile hit by every Gaussian of a wave: per-wave counts of 64 in adjacent packed halves, in all 16 tiles; one and two
# chunks of the tile sort (768 Gaussians) plus one
@pytest.mark.parametrize("N", [769, 1537])
def test_every_gaussian_covers_every_tile(N):
    act, cam = covering_scene(N)
    out_o, so = U.oracle_forward(act, cam, [0, 0, 0])
    vis = so.radii > 0
    assert int(vis.sum()) > N - 64 and int(vis[:768].sum()) > 704, int(vis.sum())
    assert bool((so.tiles[vis] == 16).all())
    _compare(act, cam, (out_o, so))


# ---- tile counts that are no multiple of 4 or 8 (the padded cursor rows, the four-tile accesses): 15, 21; 60; and 2550 tiles —
# more than 3 x 768, so the fourth round of the scatter kernel's scan runs
@pytest.mark.parametrize("H,W,T", [(48, 80, 15), (48, 112, 21), (96, 160, 60), (800, 816, 2550)])
def test_tile_counts_off_the_multiples_of_four(H, W, T):
    sc, act, cam = U.activated_scene(2049, 8, 45, H, W, scale=0.03)
    if T == 2550:  # (the cloud spread out and moved towards the image's last tile rows)
        act["means3D"] *= 1.6
        act["means3D"][:, 1] -= 0.7
    out_o, so = U.oracle_forward(act, cam, [0, 0, 0])
    assert so.ranges.shape[0] == T
    hit = so.ranges.view(np.uint32).reshape(T, 2)
    assert int((hit[:, 1] > hit[:, 0]).sum()) > T // 4  # (the lists are spread over the grid)
    if T == 2550:
        assert int((hit[3 * 768:, 1] > hit[3 * 768:, 0]).sum()) > 0  # (the fourth round has lists of its own)
    _compare(act, cam, (out_o, so))


# ---- chunk counts around the scans' segment counts: 1, 17, 33 and 65 chunks of the depth sort (2048 keys each); the tile sort's
# chunks of 768 Gaussians at these sizes — 1, 43, 86, 171 — fall on both sides of 16, 32 and 64 as well
@pytest.mark.parametrize("N,chunks", [(1, 1), (2048 * 16 + 1, 17), (2048 * 32 + 1, 33), (2048 * 64 + 1, 65)])
def test_chunk_counts_around_the_scan_segments(N, chunks):
    assert (N + 2047) // 2048 == chunks
    sc, act, cam = U.activated_scene(N, 8, 46, 64, 64, scale=0.012)
    so, s = _compare(act, cam)
    assert int(s.counters[2]) == 0


# ---- the third pass (its cursor table shares the helpers) and the two-level tile sort (it shares the chunk scan)
def test_third_pass_of_the_depth_sort():
    sc, act, cam = U.activated_scene(4097, 8, 47, 96, 160, scale=0.03, radius=2.0)
    out_o, so = U.oracle_forward(act, cam, [0, 0, 0])
    top = so.depths[so.radii > 0].view(np.uint32) >> 24
    assert top.min() != top.max()
    so, s = _compare(act, cam, (out_o, so))
    assert int(s.counters[2]) == 1


def test_two_level_tile_sort():
    from riggs_amd import _lib as L
    sc, act, cam = U.activated_scene(2049, 8, 48, 96, 160, scale=0.03)
    try:
        L.set_option("bin_grouped", 1)
        _compare(act, cam)
    finally:
        L.set_option("bin_grouped", -1)
