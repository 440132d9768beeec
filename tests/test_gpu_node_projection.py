"""The node projection term of stage 1 (train_gui.py:1133-1139): ``riggs_amd.loss.node_projection_loss`` — the implementation of
the skeleton projection loss (csrc/skel_loss.hip) over another point set, the nodes themselves — against the reference's goldens
and a float64 restatement, and against ``cal_skeleton_loss`` on a skeleton whose sample points are the same nodes.

Bounds: loss 1e-5 relative; gradient 1e-4 of its largest entry, per element."""
import os

import numpy as np
import pytest
import torch

from tests import node_projection_ref as NR

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NODEPROJ = ["nodeproj_m512_p700", "nodeproj_m33_p90_K"]


class _Cam:
    def __init__(self, z, device="cuda"):
        self.world_view_transform = torch.from_numpy(np.asarray(z["world_view_transform"], np.float32)).to(device)
        self.FoVx, self.FoVy = float(z["FoVx"]), float(z["FoVy"])
        self.image_height, self.image_width = int(z["image_height"]), int(z["image_width"])
        self.K = z["K"] if np.size(z["K"]) else None
        self.thinned = torch.from_numpy(np.asarray(z["thinned"], np.float32)).to(device)


def _intr(z):
    return NR.intrinsics(float(z["FoVx"]), float(z["FoVy"]), int(z["image_height"]), int(z["image_width"]), z["K"])


@pytest.mark.parametrize("name", NODEPROJ)
def test_float64_restatement_is_pinned_by_the_reference_goldens(name):
    """(no GPU) the projection of tests/node_projection_ref.py is the reference's own ``project_nodes_to_2d_elements``, and its
    chamfer reproduces the golden's loss and gradient."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    fx, fy, cx, cy = _intr(z)
    if np.size(z["K"]):
        assert (cx, cy) == (float(z["K"][0, 2]), float(z["K"][1, 2]))
    proj = NR.project(torch.from_numpy(z["d_nodes"].astype(np.float64)), torch.from_numpy(z["world_view_transform"].astype(np.float64)),
                      fx, fy, cx, cy).numpy()
    assert np.abs(proj - z["projected"]).max() <= 2e-6 * np.abs(z["projected"]).max()  # (the golden is float32)
    loss, g = NR.node_projection_loss(z["d_nodes"], z["world_view_transform"], fx, fy, cx, cy, z["thinned"])
    assert abs(loss - float(z["loss"])) <= 1e-5 * float(z["loss"])
    assert np.abs(g - z["grad_nodes"]).max() <= 1e-4 * np.abs(z["grad_nodes"]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NODEPROJ)
def test_node_projection_loss_matches_the_reference_golden(name):
    from riggs_amd.loss import node_projection_loss
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cam = _Cam(z)
    nodes = torch.from_numpy(z["d_nodes"]).cuda().requires_grad_(True)
    loss = node_projection_loss(nodes, cam)
    (2.5 * loss).backward()
    print(name, "loss", loss.item(), "golden", float(z["loss"]))
    g = nodes.grad.cpu().numpy() / 2.5
    print(name, "grad err / max", np.abs(g - z["grad_nodes"]).max() / np.abs(z["grad_nodes"]).max())
    assert abs(loss.item() - float(z["loss"])) <= 1e-5 * float(z["loss"])
    assert np.abs(g - z["grad_nodes"]).max() <= 1e-4 * np.abs(z["grad_nodes"]).max()
    # deterministic: no float atomics anywhere
    n2 = torch.from_numpy(z["d_nodes"]).cuda().requires_grad_(True)
    l2 = node_projection_loss(n2, cam)
    (2.5 * l2).backward()
    assert l2.item() == loss.item() and torch.equal(n2.grad, nodes.grad)


def _random_case(M, P, seed, with_K):
    rng = np.random.default_rng(seed)
    nodes = (0.5 * rng.standard_normal((M, 3))).astype(np.float32)
    view = np.eye(4, dtype=np.float32)
    view[3, :3] = [0.1, -0.05, 3.5]  # row-vector convention: translation in the last row
    H, W = 200, 260
    K = np.array([[300.0, 0, W / 2 + 3.5], [0, 300.0, H / 2 - 2.25], [0, 0, 1]]) if with_K else np.zeros((0, 0))
    z = dict(world_view_transform=view, FoVx=0.7, FoVy=0.55, image_height=H, image_width=W, K=K,
             thinned=np.stack([rng.integers(0, H, P), rng.integers(0, W, P)], -1).astype(np.float32))
    return nodes, z


# one node; one pixel; sizes beyond one 64-query block and one 256-candidate LDS slice in either direction; a camera with K
@pytest.mark.gpu
@pytest.mark.parametrize("M,P,seed,with_K", [(1, 40, 1, False), (7, 1, 2, False), (300, 1100, 3, True), (65, 257, 4, False)])
def test_node_projection_loss_against_float64(M, P, seed, with_K):
    from riggs_amd.loss import camera_intrinsics, node_projection_loss
    nodes, z = _random_case(M, P, seed, with_K)
    cam = _Cam(z)
    intr = camera_intrinsics(cam)
    assert intr == tuple(float(v) for v in _intr(z))
    want, g = NR.node_projection_loss(nodes, z["world_view_transform"], *intr, z["thinned"])
    x = torch.from_numpy(nodes).cuda().requires_grad_(True)
    loss = node_projection_loss(x, cam)
    loss.backward()
    err = np.abs(x.grad.cpu().numpy() - g).max() / np.abs(g).max()
    print("M", M, "P", P, "loss", loss.item(), "float64", want, "grad err / max", err)
    assert abs(loss.item() - want) <= 1e-5 * want
    assert err <= 1e-4
    # weight: (loss, weight * loss), either root or both differentiable — the contract of cal_skeleton_loss
    w = torch.tensor(0.37, device="cuda")
    x2 = torch.from_numpy(nodes).cuda().requires_grad_(True)
    l2, wl2 = node_projection_loss(x2, cam, weight=w)
    assert l2.item() == loss.item() and wl2.item() == pytest.approx(0.37 * loss.item(), rel=1e-6)
    torch.autograd.backward([l2, wl2], [torch.ones((), device="cuda")] * 2)
    assert np.abs(x2.grad.cpu().numpy() - 1.37 * g).max() <= 1e-4 * 1.37 * np.abs(g).max()
    # pixel_count: ``thinned`` as a buffer of fixed capacity whose first rows are the frame's
    if P > 1:
        count = P - P // 3
        want_c, g_c = NR.node_projection_loss(nodes, z["world_view_transform"], *intr, z["thinned"], pixel_count=count)
        x3 = torch.from_numpy(nodes).cuda().requires_grad_(True)
        l3 = node_projection_loss(x3, cam, pixel_count=torch.tensor(count, dtype=torch.int32, device="cuda"))
        l3.backward()
        assert abs(l3.item() - want_c) <= 1e-5 * want_c
        assert np.abs(x3.grad.cpu().numpy() - g_c).max() <= 1e-4 * np.abs(g_c).max()


# a star skeleton sampled at t = 1 puts the bone form's points (1 child + 0 root) on joints 1..J-1 exactly: both forms then run
# the same point set through the same nearest-neighbour, reduction and point-gradient code.  One point, one pixel; one past a
# 64-query block and a 256-candidate slice in both directions; several blocks with a K camera; pixel_count; weight.
@pytest.mark.gpu
@pytest.mark.parametrize("P,M,seed,with_K,counted,weighted", [(1, 1, 11, False, False, False), (65, 257, 12, False, False, False),
                                                              (300, 40, 13, True, False, False), (65, 257, 14, False, True, False),
                                                              (300, 40, 15, True, False, True)])
def test_bone_form_on_a_star_skeleton_is_the_node_form(P, M, seed, with_K, counted, weighted):
    from riggs_amd.loss import cal_skeleton_loss, node_projection_loss
    nodes, z = _random_case(P + 1, M, seed, with_K)
    cam = _Cam(z)
    kw = {}
    if counted:
        kw["pixel_count"] = torch.tensor(M - M // 3, dtype=torch.int32, device="cuda")
    if weighted:
        kw["weight"] = torch.tensor(0.37, device="cuda")
    xb = torch.from_numpy(nodes).cuda().requires_grad_(True)
    xn = torch.from_numpy(nodes).cuda().requires_grad_(True)
    lb = cal_skeleton_loss(xb, torch.zeros(P + 1, dtype=torch.int32), cam, t=torch.tensor([1.0], device="cuda"), **kw)
    ln = node_projection_loss(xn[1:], cam, **kw)
    if weighted:
        assert torch.equal(lb[0], ln[0]) and torch.equal(lb[1], ln[1])
        lb, ln = lb[0] + lb[1], ln[0] + ln[1]
    else:
        assert torch.equal(lb, ln)
    lb.backward()
    ln.backward()
    gb, gn = xb.grad.cpu().numpy(), xn.grad.cpu().numpy()
    bound = 1e-4 * np.abs(gn).max()
    print("P", P, "M", M, "loss", lb.item(), "largest |bone - node| gradient", np.abs(gb[1:] - gn[1:]).max(), "root", np.abs(gb[0]).max(),
          "bound", bound)
    assert np.all(gn[0] == 0)  # (the slice's own backward: joint 0 is no node of the node form)
    assert np.abs(gb[1:] - gn[1:]).max() <= bound
    assert np.abs(gb[0]).max() <= bound


@pytest.mark.gpu
def test_node_projection_loss_rejects_bad_inputs():
    from riggs_amd import _lib as L
    from riggs_amd.loss import node_projection_loss
    nodes, z = _random_case(5, 9, 5, False)
    cam = _Cam(z)
    with pytest.raises(L.RiggsHipError):
        node_projection_loss(torch.from_numpy(nodes), cam)  # a host tensor
    with pytest.raises(L.RiggsHipError):
        node_projection_loss(torch.zeros(0, 3, device="cuda"), cam)
    cam.thinned = torch.zeros(0, 2, device="cuda")
    with pytest.raises(L.RiggsHipError):
        node_projection_loss(torch.from_numpy(nodes).cuda(), cam)
