"""Skeletons of 65..256 joints without a GPU: SkeletonWarp's construction and state-dict layout against the reference's
(tests/golden/wideskel_state_dict_layout.json), the 256-joint bound, and the CPU oracle against the wide-skeleton golden
vectors (tests/golden/make_wideskel_golden.py)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from oracle import deform_ref as O
from riggs_amd.skeleton import SkeletonWarp

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WIDE = sorted(p for p in glob.glob(os.path.join(GOLD, "wideskel_*.npz")) if "posemlp" not in p)


def T(a):
    return torch.from_numpy(np.asarray(a))


def tree(J, seed=0):
    g = torch.Generator().manual_seed(seed)
    parents = torch.full((J,), -1, dtype=torch.long)
    for i in range(1, J):
        parents[i] = int(torch.randint(0, i, (1,), generator=g))
    return torch.rand(J, 3, generator=g), parents


@pytest.mark.parametrize("J", [65, 128, 200, 256])
def test_skeleton_warp_builds_with_the_reference_state_dict_layout(J):
    layout = json.load(open(os.path.join(GOLD, "wideskel_state_dict_layout.json")))[str(J)]
    joints, parents = tree(J)
    sw = SkeletonWarp(joints=joints, parent_indices=parents, K=-1, hyper_dim=8)
    mine = {k: list(v.shape) for k, v in sw.state_dict().items()}
    assert mine == layout
    assert list(sw.nodes.shape) == [J, 11] and list(sw._node_radius.shape) == [J]
    assert list(sw.pose_net.rotation_predictor.weight.shape)[0] + 3 == 4 * J + 3
    assert list(sw.skinning_weight_mlp.weight_predict.weight.shape)[0] == J - 1


def test_more_than_256_joints_is_an_error():
    joints, parents = tree(257)
    with pytest.raises(ValueError):
        SkeletonWarp(joints=joints, parent_indices=parents, K=-1, hyper_dim=8)


@pytest.mark.parametrize("path", WIDE, ids=[os.path.basename(p)[:-4] for p in WIDE])
def test_oracle_reproduces_the_wide_skeleton_fixtures(path):
    g = np.load(path)
    joints, parents = T(g["joints"]), T(g["parents"])
    q = T(g["local_rot"]).clone().requires_grad_(True)
    gt = T(g["global_trans"]).clone().requires_grad_(True)
    rho = T(g["node_radius_log"]).clone().requires_grad_(True)
    mask = T(g["motion_mask"]).clone().requires_grad_(True)
    x = T(g["x"])
    K = int(g["K"])
    R = O.quaternion_to_matrix(q)
    posed, G = O.fk_chain(R, joints, parents)
    np.testing.assert_allclose(G.detach().numpy(), g["transforms"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(posed.detach().numpy(), g["posed"], rtol=0, atol=2e-6)
    w, d2, idx = O.skin_weights(x, joints, parents, rho, K)
    assert np.array_equal(idx.numpy(), g["nn_idx"])
    np.testing.assert_allclose(w.detach().numpy(), g["nn_weight"], rtol=1e-5, atol=1e-7)
    out = O.deform_by_pose(x, joints, parents, rho, q, gt, mask, K)
    for k in ("d_xyz", "d_rotation", "d_scaling", "d_nodes"):
        np.testing.assert_allclose(out[k].detach().numpy(), g[k], rtol=0, atol=2e-6, err_msg=k)
    loss = (out["d_xyz"] * T(g["g_xyz"])).sum() + (out["d_rotation"] * T(g["g_rot"])).sum() \
        + (out["d_nodes"] * T(g["g_nodes"])).sum()
    loss.backward()
    for got, key in ((q.grad, "grad_local_rot"), (gt.grad, "grad_global_trans"), (rho.grad, "grad_node_radius"),
                     (mask.grad, "grad_motion_mask")):
        ref = g[key]
        scale = max(1.0, float(np.abs(ref).max()))
        np.testing.assert_allclose(got.numpy(), ref, rtol=1e-4, atol=2e-5 * scale, err_msg=key)


def test_posemlp_fixture_is_128_joints_wide():
    g = np.load(os.path.join(GOLD, "wideskel_posemlp_j128.npz"))
    assert int(g["J"]) == 128 and g["rotation"].shape == (4 * 128,)
