"""Two groups of checks for the kernels whose loads were regrouped into single round trips.

The sorts (csrc/binning.hip): the depth sort's count and scatter kernels read their elements at clamped indices in one batch, the tile
sort's count kernel reads a rectangle with one load, and its scatter kernel asks for its first batch, the tile counts and its table
row at its entry.  A slip shows in the instance list: list, tile keys and ranges are compared bit for bit with the oracle's 64-bit
(tile | depth) key sort (tests/gpu_util.py: compare_forward_state) on both routes of the depth sort, with culled Gaussians, on
ragged and multi-chunk sizes and through either tile sort.

The bone table (csrc/deform.hip): the skinning forward leaves its staged bone records with the caller and the backward stages from
them; no bit of any output may change."""
import numpy as np
import pytest
import torch

from riggs_amd.rasterizer import saved_views
from tests import gpu_util as U

pytestmark = pytest.mark.gpu


def _check(N, H, W, seed=41, scale=0.03, **camkw):
    sc, act, cam = U.activated_scene(N, 8, seed, H, W, scale=scale, **camkw)
    out_o, so = U.oracle_forward(act, cam, [0, 0, 0])
    color, radii, depth, alpha, s = U.hip_forward(act, cam, [0, 0, 0])
    U.compare_forward_state(so, saved_views(s), out_o, color, depth, alpha, radii)
    return so, s


# 2048 keys are a workgroup of the depth sort and 1024 Gaussians one of the tile sort: one short chunk, a chunk but one, a chunk
# and one, two chunks and one; 64 x 64 is 16 tiles, 160 x 96 is 10 x 6 with a ragged right column of pixels
@pytest.mark.parametrize("H,W", [(64, 64), (96, 160)])
@pytest.mark.parametrize("N", [1, 63, 2047, 2049, 4097])
def test_instance_list_equals_the_oracles_at_chunk_edges(N, H, W):
    so, s = _check(N, H, W)
    assert int(s.counters[2]) == 0  # (every depth in [2, 8): the two-pass route)


def test_instance_list_through_the_third_pass():
    """Depths on both sides of 2.0 differ in their top byte: the third pass runs and it is the one that writes the order."""
    so, s = _check(4097, 96, 160, radius=2.0)  # (the camera two units from the cloud's centre)
    assert int(s.counters[2]) == 1
    top = so.depths[so.radii > 0].view(np.uint32) >> 24
    assert top.min() != top.max()


def test_instance_list_with_culled_gaussians():
    """A camera close to the cloud (every depth in [0.5, 2): the two-pass route): the Gaussians beside the frustum keep an empty
    rectangle, which travels through the sort like any other and adds no instance."""
    so, s = _check(4097, 96, 160, radius=1.0, scale=0.01)
    assert int(s.counters[2]) == 0
    culled = int((so.radii == 0).sum())
    assert 1000 < culled < 3500, culled


def test_instance_list_through_the_two_level_tile_sort():
    from riggs_amd import _lib as L
    try:
        L.set_option("bin_grouped", 1)
        _check(2049, 96, 160)
    finally:
        L.set_option("bin_grouped", -1)


# ---- the bone table: the skinning forward leaves its staged bone records with the caller, the backward stages from them
def _skin_inputs(N, J, mod):
    from riggs_amd import synth
    sc = synth.make_scene(N, J, 11 + J)
    g = torch.Generator().manual_seed(100 * J + N)
    dev = {k: sc[k].float().contiguous().cuda() for k in ("xyz", "joints", "node_radius", "local_rotation", "global_trans")}
    dev["parents"] = torch.as_tensor(sc["parents"]).to(torch.int32).cuda()
    dev["mask"] = torch.rand(N, generator=g).cuda()
    dev["mod"] = torch.rand(N, J - 1, generator=g).cuda() if mod else None
    return dev, g


def _forward(lib, L, d, N, J, table, fk):
    """riggs_lbs_forward_fk, or riggs_fk_forward + riggs_lbs_forward: (transforms, node_rot, d_nodes, d_xyz, d_rotation)"""
    tr, nr, dn, dx, dr = (torch.full(sh, float("nan"), device="cuda") for sh in ((J, 12), (J, 4), (J, 3), (N, 3), (N, 4)))
    if fk:
        L.check(lib.riggs_lbs_forward_fk(N, J, -1, d["xyz"].data_ptr(), d["joints"].data_ptr(), d["parents"].data_ptr(),
                                         d["node_radius"].data_ptr(), d["local_rotation"].data_ptr(), d["global_trans"].data_ptr(),
                                         d["mask"].data_ptr(), L.ptr(d["mod"]), tr.data_ptr(), nr.data_ptr(), dn.data_ptr(),
                                         dx.data_ptr(), dr.data_ptr(), L.ptr(table), L.stream_ptr()), "riggs_lbs_forward_fk")
    else:
        L.check(lib.riggs_fk_forward(J, d["local_rotation"].data_ptr(), d["joints"].data_ptr(), d["parents"].data_ptr(),
                                     d["global_trans"].data_ptr(), tr.data_ptr(), nr.data_ptr(), dn.data_ptr(), L.stream_ptr()),
                "riggs_fk_forward")
        L.check(lib.riggs_lbs_forward(N, J, -1, d["xyz"].data_ptr(), d["joints"].data_ptr(), d["parents"].data_ptr(),
                                      d["node_radius"].data_ptr(), tr.data_ptr(), nr.data_ptr(), d["global_trans"].data_ptr(),
                                      d["mask"].data_ptr(), L.ptr(d["mod"]), dx.data_ptr(), dr.data_ptr(), None, None, L.ptr(table),
                                      L.stream_ptr()), "riggs_lbs_forward")
    torch.cuda.synchronize()
    return tr, nr, dn, dx, dr


def _backward(lib, L, d, N, J, tr, nr, gx, gr, table):
    dG, drho, dgt, dm = (torch.full(sh, float("nan"), device="cuda") for sh in ((J, 12), (J,), (3,), (N,)))
    dw = torch.full((N, J - 1), float("nan"), device="cuda") if d["mod"] is not None else None
    ws = torch.empty(lib.riggs_lbs_backward_workspace_bytes(N, J), dtype=torch.uint8, device="cuda")
    L.check(lib.riggs_lbs_backward_table(N, J, -1, d["xyz"].data_ptr(), d["joints"].data_ptr(), d["parents"].data_ptr(),
                                         d["node_radius"].data_ptr(), tr.data_ptr(), nr.data_ptr(), d["global_trans"].data_ptr(),
                                         d["mask"].data_ptr(), L.ptr(d["mod"]), gx.data_ptr(), gr.data_ptr(), dG.data_ptr(),
                                         drho.data_ptr(), dgt.data_ptr(), dm.data_ptr(), L.ptr(dw), L.ptr(table), ws.data_ptr(),
                                         L.stream_ptr()), "riggs_lbs_backward_table")
    torch.cuda.synchronize()
    return [t for t in (dG, drho, dgt, dm, dw) if t is not None]


@pytest.mark.parametrize("mod", [False, True])
@pytest.mark.parametrize("N", [1, 255, 1025])
@pytest.mark.parametrize("J", [2, 24, 64])
def test_bone_table_changes_no_bit_forward_or_backward(J, N, mod):
    """Forward outputs with and without a table, through both entry points; backward gradients staged from the forward's table
    against the ones rebuilt from joints / parents / radii / transforms (table NULL), for dense and 5 %-sparse cotangents: all bit
    for bit.  (The table holds what stage_bones computes, so the two backwards run the same arithmetic on the same records.  At
    N = 1025 three and more waves of a workgroup contribute: their sums meet in wave order — a slot per wave in LDS —, where LDS
    atomics in arrival order made two runs of the SAME call differ in the last place of dG.)"""
    from riggs_amd import _lib as L
    lib = L.lib()
    d, g = _skin_inputs(N, J, mod)
    table = torch.zeros(int(lib.riggs_lbs_bone_table_bytes()), dtype=torch.uint8, device="cuda")
    for fk in (True, False):
        plain = _forward(lib, L, d, N, J, None, fk)
        table.zero_()
        with_table = _forward(lib, L, d, N, J, table, fk)
        for a, b in zip(plain, with_table):
            assert not torch.isnan(a).any() and torch.equal(a, b)
        assert int(table[: 112 * (J - 1)].view(torch.int32).ne(0).sum()) > 0, "the forward left no bone records"
        assert int(table[112 * (J - 1):].ne(0).sum()) == 0, "the forward wrote behind the J - 1 records"
    tr, nr = with_table[0], with_table[1]
    for keep in (1.0, 0.05):
        m = (torch.rand(N, 1, generator=g) < keep).float()
        gx, gr = (torch.randn(N, 3, generator=g) * m).cuda(), (torch.randn(N, 4, generator=g) * m).cuda()
        ref = _backward(lib, L, d, N, J, tr, nr, gx, gr, None)
        got = _backward(lib, L, d, N, J, tr, nr, gx, gr, table)
        for a, b in zip(ref, got):
            assert not torch.isnan(a).any() and torch.equal(a, b), (keep, float((a - b).abs().max()))


def test_autograd_nodes_hand_the_forwards_table_to_the_backward():
    """SkeletonWarp's two nodes (pose given / pose from the PoseMLP) save the table and stage the backward from it: the gradients
    equal the ones of the same backward without a table, which riggs_lbs_backward (the NULL-table wrapper) gives."""
    from riggs_amd import _lib as L
    from riggs_amd import skeleton as S
    from riggs_amd import synth
    N, J = 511, 24  # (two contributing waves per workgroup: the backward's sums are reproducible to the bit)
    sc = synth.make_scene(N, J, 7)
    seen = []
    orig = S._skinning_backward

    def spy(*a, **k):
        seen.append((S._BONE_TABLE_MAX_J > 0, k.get("bone_table") is not None))
        return orig(*a, **k)
    sw = S.SkeletonWarp(joints=sc["joints"], parent_indices=sc["parents"], K=-1, hyper_dim=8, use_skinning_weight_mlp=False,
                        use_template_offsets=False).cuda()
    sw._node_radius.data = sc["node_radius"].cuda()
    g = torch.Generator().manual_seed(3)
    gx, gr = torch.randn(N, 3, generator=g).cuda(), torch.randn(N, 4, generator=g).cuda()
    grads = {}
    S._skinning_backward = spy
    try:
        for with_table in (True, False):
            keep = S._BONE_TABLE_MAX_J
            S._BONE_TABLE_MAX_J = keep if with_table else 0  # (0: no table is allocated, the library rebuilds the records)
            try:
                q = sc["local_rotation"].cuda().requires_grad_(True)
                sw._node_radius.grad = None
                h = sw.deform_by_pose(sc["xyz"].cuda(), {"local_rotation": q, "global_trans": sc["global_trans"].cuda()},
                                      sc["motion_mask"].cuda())
                ((h["d_xyz"] * gx).sum() + (h["d_rotation"] * gr).sum()).backward()
                f = sw(sc["xyz"].cuda(), sw.expand_time(torch.tensor([0.41], device="cuda")), motion_mask=sc["motion_mask"].cuda())
                for p in sw.pose_net.parameters():
                    p.grad = None
                ((f["d_xyz"] * gx).sum() + (f["d_rotation"] * gr).sum()).backward()
                torch.cuda.synchronize()
                grads[with_table] = [q.grad.clone(), sw._node_radius.grad.clone()] + [p.grad.clone() for p in sw.pose_net.parameters()
                                                                                      if p.grad is not None]
            finally:
                S._BONE_TABLE_MAX_J = keep
    finally:
        S._skinning_backward = orig
    # (the ctypes nodes go through _skinning_backward; the pose-net node may be the C++ extension's, which takes the same table)
    assert len(seen) >= 2 and all(want == got for want, got in seen), seen
    assert len(grads[True]) == len(grads[False]) > 2
    for a, b in zip(grads[True], grads[False]):
        assert torch.equal(a, b)
