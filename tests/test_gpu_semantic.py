"""GPU: the nodes' semantic labels (csrc/semantic.hip through riggs_amd.skeleton_init.node_semantic_labels) against the NumPy
restatement tests/semantic_ref.py — ``labels`` and ``median`` EXACTLY — and ``precompute_deformations(symmetry=True)`` end to end.

A truncation could flip where a projection lies within fp32 rounding of an integer, so every case first checks, in float64 and
over ALL (frame, node) pairs, that no projection coordinate is nearer than 1e-3 px to an integer (the scenes of semantic_ref put
them on a quarter-pixel lattice, 1 / 8 px or more from any integer); no pair is excluded from the comparison."""
import numpy as np
import pytest
import torch

from tests import semantic_ref as SR

pytestmark = pytest.mark.gpu

# F: 1; 2 (an even count: the LOWER median); 5; 65 and 130 (past one wave, and past the node tile's changes at 64 and 128 frames);
# 1024 (the limit, 16 nodes per workgroup).  M: 1; 64; 65; 513 (several workgroups and a ragged last tile at every tile size).
FRAMES = (1, 2, 5, 65, 130, 1024)
NODES = (1, 64, 65, 513)
_SCENES = {}


def scene(F, M, null_every=0, null_keep=0):
    """(d_nodes, cameras, labels, median, hits) of one case: computed once, shared, not modified."""
    key = (F, M, null_every, null_keep)
    if key not in _SCENES:
        d_nodes, cameras = SR.scene(F, M, seed=F + 3 * M, null_every=null_every, null_keep=null_keep)
        _SCENES[key] = (d_nodes, cameras) + SR.labels_and_median(d_nodes, cameras, np.float64)
    return _SCENES[key]


def device_cameras(cameras):
    """The cameras with their tensors as torch tensors: the view on the device, the maps on the HOST as int64 for every other
    camera (moved and cast by node_semantic_labels) and on the device as int32 for the rest."""
    out = []
    for f, c in enumerate(cameras):
        seg = c.semantic_seg
        if seg is not None:
            seg = torch.from_numpy(seg).long() if f % 2 else torch.from_numpy(seg).cuda()
        d = SR.Camera(c.world_view_transform, c.image_height, c.image_width, 1.0, 1.0, seg, None if c.K is None else torch.from_numpy(c.K))
        d.FoVx, d.FoVy = c.FoVx, c.FoVy
        d.world_view_transform = torch.from_numpy(c.world_view_transform).cuda()
        out.append(d)
    return out


def run(d_nodes, cameras):
    from riggs_amd import skeleton_init as SI
    labels, median = SI.node_semantic_labels(torch.from_numpy(d_nodes).cuda(), device_cameras(cameras))
    assert labels.is_cuda and labels.dtype == torch.float32 and labels.shape == d_nodes.shape[:2]
    assert median.is_cuda and median.dtype == torch.int32 and median.shape == (d_nodes.shape[1],)
    return labels.cpu().numpy(), median.cpu().numpy()


def check(F, M, null_every=0, null_keep=0):
    d_nodes, cameras, ref_labels, ref_median, hits = scene(F, M, null_every, null_keep)
    assert SR.distance_to_integer(d_nodes, cameras) > 1e-3  # every pair, cameras without a map included
    labels32, median32, _ = SR.labels_and_median(d_nodes, cameras, np.float32)
    assert np.array_equal(labels32, ref_labels) and np.array_equal(median32, ref_median)  # float32 and float64 agree on the rule
    labels, median = run(d_nodes, cameras)
    assert np.array_equal(labels, ref_labels)
    assert np.array_equal(median, ref_median)
    return hits


@pytest.mark.parametrize("M", NODES)
@pytest.mark.parametrize("F", FRAMES)
def test_labels_and_median_equal_the_restatement(F, M):
    check(F, M)
    _, cameras, ref_labels, _, _ = scene(F, M)
    if F >= 5:
        assert {(c.image_height, c.image_width) for c in cameras} >= {(7, 5), (40, 64)} and any(c.K is not None for c in cameras)
    if F * M >= 64:
        assert ref_labels.max() > 2 ** 19 and ref_labels.min() < 0  # large and negative labels are read


def test_every_clamp_is_hit():
    hits = sum(scene(F, 65)[4] for F in (5, 65))
    assert all(int(h) > 0 for h in hits), hits  # rows >= H, columns >= W, coordinates < 0
    # ... and truncation toward zero is not floor: some projection lies in (-1, 0), which is pixel 0 without the < 0 clamp
    d_nodes, cameras = scene(65, 65)[:2]
    assert any(((p > -1) & (p < 0)).any() for p in (SR.project(c, d_nodes[f], np.float64) for f, c in enumerate(cameras)))


@pytest.mark.parametrize("F, M, null_every, null_keep", [(5, 65, 3, 0), (65, 64, 4, 0), (130, 65, 3, 0), (6, 513, 3, 1), (65, 65, 4, 1),
                                                         (1024, 65, 5, 1), (2, 64, 2, 0), (1, 64, 1, 1)])
def test_cameras_without_a_map_give_zero_rows(F, M, null_every, null_keep):
    """Without a map in the majority of the cameras (the median is then 0 wherever it is not negative) and in a minority; with
    one of two, and with the only one."""
    check(F, M, null_every, null_keep)
    _, cameras, ref_labels, ref_median, _ = scene(F, M, null_every, null_keep)
    missing = [f for f, c in enumerate(cameras) if c.semantic_seg is None]
    assert 0 < len(missing) and (len(missing) >= F / 2) == (null_keep == 0 or F == 1)
    assert not ref_labels[missing].any()
    if null_keep:
        assert F == 1 or ref_median.any()
    else:
        assert (ref_median <= 0).all()


def test_the_median_is_the_lower_one_and_matches_torch():
    """Two frames: the lower median is the smaller label, not the mean and not the upper; torch.median on the kernel's own
    labels gives the kernel's median at every F."""
    for F, M in ((2, 64), (5, 65), (130, 64)):
        _, _, ref_labels, ref_median, _ = scene(F, M)
        assert np.array_equal(torch.median(torch.from_numpy(ref_labels), dim=0).values.int().numpy(), ref_median)
    _, _, ref_labels, ref_median, _ = scene(2, 64)
    assert np.array_equal(ref_median, ref_labels.min(axis=0).astype(np.int32)) and (ref_labels[0] != ref_labels[1]).any()


def test_a_projection_that_is_not_finite_reads_pixel_0_0():
    d_nodes, cameras = SR.scene(3, 8, seed=5)
    d_nodes = d_nodes.copy()
    view = cameras[1].world_view_transform.astype(np.float64)
    d_nodes[1, 2] = (np.array([0.5, 0.25, 0.0]) - view[3, :3]) @ view[:3, :3].T  # z = 0 in camera 1: a division by zero
    d_nodes[2, 5] = np.nan
    labels, median = run(d_nodes, cameras)
    assert labels[1, 2] == np.float32(cameras[1].semantic_seg[0, 0]) and labels[2, 5] == np.float32(cameras[2].semantic_seg[0, 0])
    keep = np.ones((3, 8), dtype=bool)
    keep[1, 2] = keep[2, 5] = False
    with np.errstate(invalid="ignore"):
        assert np.array_equal(labels[keep], SR.labels_and_median(np.nan_to_num(d_nodes, nan=1.0), cameras)[0][keep])


def test_rejected_shapes_return_errors_without_a_launch():
    from riggs_amd import _lib as L
    from riggs_amd import skeleton_init as SI
    lib = L.lib()
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    for F, M in ((0, 4), (1025, 4), (4, 0), (4, 65537), (-1, 4)):
        assert lib.riggs_node_semantic_labels(F, M, p, p, p, p, L.stream_ptr()) != 0
        assert b"riggs_node_semantic_labels" in lib.riggs_last_error()
    assert lib.riggs_node_semantic_labels(1, 1, None, p, p, p, L.stream_ptr()) != 0 and b"NULL" in lib.riggs_last_error()
    torch.cuda.synchronize()
    assert not buf.any()  # nothing ran
    cam = SR.scene(1, 1, seed=1)[1]
    with pytest.raises(L.RiggsHipError):
        SI.node_semantic_labels(torch.zeros(0, 4, 3, device="cuda"), [])
    with pytest.raises(L.RiggsHipError):
        SI.node_semantic_labels(torch.zeros(1, 0, 3, device="cuda"), device_cameras(cam))
    with pytest.raises(L.RiggsHipError):
        SI.node_semantic_labels(torch.zeros(2, 4, 3, device="cuda"), device_cameras(cam))  # one camera for two frames
    with pytest.raises(L.RiggsHipError):
        SI.node_semantic_labels(torch.zeros(1, 4, 3), device_cameras(cam))  # host nodes


def test_the_launch_is_capturable():
    """No allocation, read-back or synchronisation in the entry: a captured launch replays on new nodes."""
    from riggs_amd import _lib as L
    d_nodes, cameras, ref_labels, ref_median, _ = scene(5, 65)
    other = SR.scene(5, 65, seed=99)
    words = L.CONSTANTS["RIGGS_SEMANTIC_CAMERA_WORDS"]
    table = np.zeros((5, words), dtype=np.uint32)
    maps = [torch.from_numpy(c.semantic_seg).cuda() for c in cameras]
    for f, c in enumerate(cameras):
        table[f, :16] = c.world_view_transform.reshape(16).view(np.uint32)
        table[f, 16:20] = np.array(SR.intrinsics(c), dtype=np.float32).view(np.uint32)
        table[f, 20:22] = (c.image_height, c.image_width)
        table[f, 22:24] = (maps[f].data_ptr() & 0xFFFFFFFF, maps[f].data_ptr() >> 32)
    table = torch.from_numpy(table.view(np.int32)).cuda()
    nodes = torch.from_numpy(other[0]).cuda()
    labels, median = torch.zeros(5, 65, device="cuda"), torch.zeros(65, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(L.lib().riggs_node_semantic_labels(5, 65, nodes.data_ptr(), table.data_ptr(), labels.data_ptr(), median.data_ptr(),
                                                   L.stream_ptr()), "riggs_node_semantic_labels")
    nodes.copy_(torch.from_numpy(d_nodes))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().numpy(), ref_labels) and np.array_equal(median.cpu().numpy(), ref_median)


def test_precompute_deformations_with_symmetry_end_to_end():
    """A ControlNodeWarp on the uneven figure's nodes with the static node network: symmetry=True with cameras extracts the tree
    of obtain_skeleton_tree(..., seg_labels=median of the cameras' labels); symmetry=True alone that of zero labels;
    symmetry=False (with or without cameras) today's tree."""
    from riggs_amd import skeleton_init as SI
    from riggs_amd.control_nodes import ControlNodeWarp, StaticNodeNetwork
    from riggs_amd.gaussian_model import GaussianModel
    from tests.test_skeleton_symmetry_cpu import fixture
    nodes = torch.from_numpy(fixture("skelsym_uneven")["nodes"])
    M, N, hyper = nodes.shape[0], 300, 2
    g = torch.Generator().manual_seed(4)
    warp = ControlNodeWarp(node_num=M, K=3, hyper_dim=hyper, with_node_weight=True, network=StaticNodeNetwork()).cuda()
    warp.nodes.data = torch.cat([nodes, 1e-2 * torch.ones(M, hyper)], -1).cuda()
    warp._node_radius.data = torch.full((M,), float(np.log(0.05)), device="cuda")
    warp._node_weight.data = torch.zeros(M, 1, device="cuda")
    xyz = nodes[torch.randint(0, M, (N,), generator=g)] + 0.02 * torch.randn(N, 3, generator=g)

    def gaussians():
        gm = GaussianModel.from_tensors(xyz, torch.rand(N, 1, 3, generator=g), torch.zeros(N, 15, 3), torch.full((N, 3), -4.0),
                                        torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(N, 1), torch.zeros(N, 1), device="cuda")
        gm.feature = torch.zeros(N, hyper, device="cuda")
        return gm

    fids = torch.tensor([0.5, 0.0, 1.0, 0.25, 0.75])
    # five cameras looking down -z from z = 3 at the figure (|x|, |y| <= 1), 32 x 32 px, the map's label = the image quadrant + 1;
    # one camera has no map.  In the order of fids.
    view = np.eye(4, dtype=np.float32)
    view[3, 2] = 3.0
    seg = (1 + (np.arange(32)[:, None] >= 16) * 2 + (np.arange(32)[None, :] >= 16)).astype(np.int32)
    cameras = [SR.Camera(view + 0.0, 32, 32, 40.0, 40.0, None if k == 3 else torch.from_numpy(np.roll(seg, k, axis=1))) for k in range(5)]
    for c in cameras:
        c.world_view_transform = torch.from_numpy(c.world_view_transform).cuda()

    info, tree, _ = SI.precompute_deformations(warp, gaussians(), fids, cameras=cameras, symmetry=True)
    order = torch.argsort(fids, stable=True).tolist()
    labels, median = SI.node_semantic_labels(info["d_nodes"], [cameras[i] for i in order])
    assert torch.equal(info["nodes_semantic_label"], labels) and labels.shape == (5, M)
    assert not labels[order.index(3)].any() and len(torch.unique(median)) >= 3  # (the camera without a map, by ITS frame)
    t = tree["template_idx"]
    want = SI.obtain_skeleton_tree(info["d_nodes"][t], info["d_nodes"], seg_labels=median, symmetry=True)
    for a, b in zip((tree["joints"], tree["parent_indices"], tree["joint_node_indices"]), want):
        assert torch.equal(a, b)

    def same(tree, want):
        return all(torch.equal(a, b) for a, b in zip((tree["joints"], tree["parent_indices"], tree["joint_node_indices"]), want))

    info0, tree0, _ = SI.precompute_deformations(warp, gaussians(), fids, symmetry=True)
    assert "nodes_semantic_label" not in info0
    assert same(tree0, SI.obtain_skeleton_tree(info["d_nodes"][t], info["d_nodes"], seg_labels=torch.zeros(M, dtype=torch.int32), symmetry=True))
    today = SI.obtain_skeleton_tree(info["d_nodes"][t], info["d_nodes"], None)
    for kwargs in ({}, {"symmetry": False}, {"cameras": cameras}):
        info1, tree1, _ = SI.precompute_deformations(warp, gaussians(), fids, **kwargs)
        assert same(tree1, today) and "nodes_semantic_label" not in info1
