"""Stage-1 node regularisers without a GPU: ControlNodeWarp carries every member the reference trainer touches
(tests/golden/stage1_surface.json), and the float64 restatement (tests/node_reg_ref.py) reproduces the reference's
cal_connectivity_from_points + cal_arap_error fixture."""
import json
import os

import numpy as np
import torch

from tests import node_reg_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_control_node_warp_has_the_stage1_surface():
    from riggs_amd.control_nodes import ControlNodeWarp
    names = json.load(open(os.path.join(GOLDEN, "stage1_surface.json")))
    assert len(names) >= 30
    cn = ControlNodeWarp(node_num=16, K=3, hyper_dim=8, is_blender=True, with_arap_loss=True, enable_densify_prune=False,
                         is_scene_static=False, hash_time=False)
    missing = [n for n in names if not (hasattr(type(cn), n) or hasattr(cn, n))]
    assert not missing, missing
    assert cn.name == "node" and cn.use_hash is False and cn.cached_nn_weight is False
    assert cn.nodes_color_visualization.shape == cn.nodes.shape
    assert "inited" in dict(cn.named_buffers())


def test_restatement_matches_reference_arap_fixture():
    z = np.load(os.path.join(GOLDEN, "stage1_arap_m64_t3.npz"))
    seq = torch.from_numpy(z["seq"])
    idx, dist = R.knn_ref(seq[0], 11, drop_first=True, least_edge_num=3, radius=0.1)
    keep = idx.reshape(-1) != -1
    assert torch.equal(idx.reshape(-1)[keep], torch.from_numpy(z["jj"]))
    assert torch.equal(torch.arange(64)[:, None].expand(64, 10).reshape(-1)[keep], torch.from_numpy(z["ii"]))
    assert torch.equal(torch.arange(10)[None].expand(64, 10).reshape(-1)[keep], torch.from_numpy(z["nn"]))
    w = torch.exp(-dist / dist.mean())
    w = w / w.sum(-1, keepdim=True)
    assert np.array_equal(np.isnan(w.numpy()), np.isnan(z["weight"])) and np.isnan(z["weight"]).any()
    s = seq.double().requires_grad_(True)
    e = R.arap_ref(s, idx, torch.arange(64))
    e.backward()
    assert abs(float(e) - float(z["arap"])) <= 1e-5 * abs(float(z["arap"]))
    g = z["grad_seq"]
    assert np.abs(s.grad.numpy() - g).max() <= 1e-4 * np.abs(g).max()
    # the fixture's unchanged-coordinate row: its rotation is the identity (S = 0)
    Rm = R.arap_rotations(seq, idx, torch.arange(64))
    assert torch.equal(Rm[5, 1], torch.eye(3, dtype=torch.float64)) and torch.equal(Rm[5, 2], torch.eye(3, dtype=torch.float64))


def test_restatement_matches_reference_arap_fixture_with_sample():
    z = np.load(os.path.join(GOLDEN, "stage1_arap_m600_t3.npz"))
    seq = torch.from_numpy(z["seq"])
    idx, _ = R.knn_ref(seq[0], 11, drop_first=True, least_edge_num=3, radius=0.1)
    keep = idx.reshape(-1) != -1
    assert torch.equal(idx.reshape(-1)[keep], torch.from_numpy(z["jj"]))
    s = seq.double().requires_grad_(True)
    e = R.arap_ref(s, idx, torch.from_numpy(z["rows"]).long())
    e.backward()
    assert abs(float(e) - float(z["arap"])) <= 1e-5 * abs(float(z["arap"]))
    assert np.abs(s.grad.numpy() - z["grad_seq"]).max() <= 1e-4 * np.abs(z["grad_seq"]).max()


def test_restatement_matches_reference_loss_fixture():
    """float64 restatement of arap_loss / elastic_loss / acc_loss at the recorded times vs the reference module"""
    z = np.load(os.path.join(GOLDEN, "stage1_losses_m300.npz"))
    M = z["nodes"].shape[0]
    for loss in ("arap", "elastic", "acc"):
        net = R.ClosedFormNodeNet().double()
        for k, p in net.named_parameters():
            p.data = torch.from_numpy(z["net_" + k]).double()
        nodes = torch.from_numpy(z["nodes"]).double().requires_grad_(True)
        radius = torch.from_numpy(z["_node_radius"]).double().requires_grad_(True)
        wl = torch.from_numpy(z["_node_weight"]).double().requires_grad_(True)
        t = torch.from_numpy(z[loss + "_t"][0]).double().reshape(-1, 1)
        T = t.shape[0] // M
        x = nodes[:, None, :3].detach().expand(M, T, 3).reshape(-1, 3)
        nt = nodes[:, None, :3].detach() + net(x=x, t=t)["d_xyz"].view(M, T, 3)
        if loss == "arap":
            idx, _ = R.knn_ref(nt[:, 0].float(), 11, drop_first=True, least_edge_num=3, radius=0.1)
            v = R.arap_ref(nt.permute(1, 0, 2), idx, torch.arange(M))
        elif loss == "elastic":
            kidx, _ = R.knn_ref(nodes.detach().float(), 3)
            w = R.graph_weight_ref(nodes, radius, wl, 8, kidx)
            v = R.elastic_ref(nt, kidx[:, 1:], w[:, 1:])
        else:
            v = R.acc_ref(nt)
        v.backward()
        assert abs(float(v) - float(z[loss])) <= 1e-5 * abs(float(z[loss])), loss
        named = list(net.named_parameters()) + [("nodes", nodes), ("_node_radius", radius), ("_node_weight", wl)]
        # scale: the tensor's largest gradient, at least 1 % of the loss's largest one (acc's gradient to B is zero in exact
        # arithmetic; the fp32 reference holds rounding noise of 3e-8 of the largest gradient there)
        gmax = max(np.abs(z[loss + "_grad_" + k]).max() for k, _ in named)
        for k, p in named:
            ref = z[loss + "_grad_" + k]
            got = p.grad.numpy() if p.grad is not None else np.zeros(ref.shape)
            assert np.abs(got - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-2 * gmax), (loss, k)
