"""GPU: the stage-2 skeleton extraction on device tensors against the reference's recorded trees (tests/golden/skelinit_*.npz),
and ``precompute_deformations`` / the stage-2 start on a small stage-1 model."""
import os

import numpy as np
import pytest
import torch

from tests import skeleton_init_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", R.SKELETON_FIXTURES)
def test_extraction_on_the_device_returns_the_recorded_tree(name):
    from riggs_amd import skeleton_init as SI
    z = R.skeleton_fixture(name)
    nodes, alld = torch.from_numpy(z["nodes"]).cuda(), torch.from_numpy(z["all_deformed"]).cuda()
    start = int(z["start"]) if nodes.shape[0] > 200 else None
    joints, parents, indices = SI.obtain_skeleton_tree(nodes, alld, None, start=start)
    assert joints.is_cuda and parents.is_cuda and indices.is_cuda
    assert joints.dtype == torch.float32 and parents.dtype == torch.int64 and indices.dtype == torch.int32
    assert np.array_equal(parents.cpu().numpy(), z["parents"])
    assert np.array_equal(indices.cpu().numpy(), z["indices"])
    assert np.array_equal(joints.cpu().numpy().view(np.uint32), z["joints"].view(np.uint32))


def test_precompute_deformations_and_the_stage2_start(tmp_path):
    from riggs_amd import skeleton_init as SI
    warp, gm = R.stage1_scene()
    fids = torch.tensor([0.8, 0.0, 0.2, 1.0, 0.4, 0.6])  # (visited in ascending order)
    xyz0 = gm.get_xyz.detach().clone()
    with torch.no_grad():
        per = [warp(xyz0, warp.expand_time(torch.tensor([float(f)], device="cuda")), feature=gm.feature, motion_mask=gm.motion_mask)
               for f in sorted(fids.tolist())]
    coverage = torch.tensor([5.0, 9.0, 1.0, 2.0, 3.0, 4.0])  # in the order of fids
    info, tree, offsets = SI.precompute_deformations(warp, gm, fids, coverage=coverage, model_path=str(tmp_path))
    t = tree["template_idx"]
    assert 0 <= t < 6 and info["d_xyz"].shape == (6, 500, 3) and info["d_nodes"].shape == (6, 64, 3)
    assert t == SI.select_key_frame(torch.stack([p["d_nodes"] for p in per]), coverage[torch.argsort(fids)])
    # the stacked outputs are the per-frame forward calls, with the template frame's d_xyz moved into the Gaussians
    assert torch.equal(offsets, per[t]["d_xyz"])
    assert torch.equal(gm.get_xyz.detach(), xyz0 + offsets)
    for f in range(6):
        assert torch.equal(info["d_xyz"][f], per[f]["d_xyz"] - offsets)
        for k in ("d_nodes", "d_rotation", "d_scaling"):
            assert torch.equal(info[k][f], per[f][k]), (k, f)
    assert float(info["d_xyz"][t].abs().max()) == 0.0
    idx = tree["joint_node_indices"]
    J = idx.shape[0]
    assert J >= 4 and tree["joints"].shape == (J, 3) and int(tree["parent_indices"][0]) == -1
    assert torch.equal(info["d_joints"], info["d_nodes"][:, idx.long()])
    # the files: the tree loads back, the OBJ has one vertex per joint and one line per bone
    back = SI.load_skeleton_tree(os.path.join(tmp_path, "skeleton_tree.npz"), device="cuda")
    assert torch.equal(back["joints"], tree["joints"]) and torch.equal(back["parent_indices"], tree["parent_indices"])
    assert torch.equal(back["joint_node_indices"], idx.long()) and back["template_idx"] == t
    rows = open(os.path.join(tmp_path, "skeleton.obj")).read().split("\n")
    assert sum(r.startswith("v ") for r in rows) == J and sum(r.startswith("l ") for r in rows) == J - 1
    # stage 2 starts from it: the joints' radii are their nodes', and one step deforms the Gaussians
    model = SI.skeleton_model_from_tree(back, stage1=warp, K=3, hyper_dim=2, use_skinning_weight_mlp=False, use_template_offsets=False)
    assert torch.equal(model.deform._node_radius.detach(), warp._node_radius.detach()[idx.long()])
    assert torch.equal(model.deform.nodes[:, :3].detach(), tree["joints"])
    out = model.step(gm.get_xyz.detach(), torch.tensor(0.3, device="cuda"), motion_mask=gm.motion_mask)
    assert out["d_xyz"].shape == (500, 3) and bool(torch.isfinite(out["d_xyz"]).all())
