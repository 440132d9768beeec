"""Readers of the skeleton-extraction and farthest-point fixtures (tests/golden/make_skeleton_init_golden.py wrote them from the
reference) and the small stage-1 scene the extraction tests share."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SKELETON_FIXTURES = ("skelinit_per12", "skelinit_per30", "skelinit_per60", "skelinit_per100", "skelinit_per30_twigs")
FPS_FIXTURES = ("fps_n70001_p64", "fps_n200_p200", "fps_n2050x2_p40", "fps_same300_p5", "fps_n1_p1")
_CACHE = {}


def skeleton_fixture(name):
    """The fixture as a dict of numpy arrays, with the inputs (``nodes`` (M, 3), ``all_deformed`` (F, M, 3) fp32) and the full
    (S, S) ``mean_distances`` put back together from their compact forms.  Read once; do not modify."""
    if name not in _CACHE:
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        grid = np.float32(z["grid"])
        z["nodes"] = z.pop("nodes_q").astype(np.float32) / grid
        z["all_deformed"] = z.pop("all_deformed_q").astype(np.float32) / grid
        tri = np.ascontiguousarray(z.pop("mean_distances_triu_bytes").T).view("<f4").ravel()
        S = len(z["sample"])
        md = np.zeros((S, S), dtype=np.float32)
        md[np.triu_indices(S, 1)] = tri
        md = md + md.T
        at = z["mean_distances_low_at"]
        md[at[:, 0], at[:, 1]] = z["mean_distances_low"]
        z["mean_distances"] = md
        _CACHE[name] = z
    return _CACHE[name]


def fps_fixture(name):
    """(points (N, 3) fp32, start, reference indices (npoint,) int64)."""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        if "lattice_int8" in z.files:
            pts = z["lattice_int8"].astype(np.float32) * np.float32(z["lattice_scale"])
        else:
            pts = z["points"]
        if name == "fps_n2050x2_p40":  # the cloud twice: every distance occurs at n and at n + 2050, in two workgroups
            pts = np.tile(pts, (2, 1))
        if name == "fps_same300_p5":
            pts = np.tile(pts, (300, 1))
        _CACHE[name] = (np.ascontiguousarray(pts, dtype=np.float32), int(z["start"]), z["indices"].astype(np.int64))
    return _CACHE[name]


def star_nodes(limbs=3, per=21, seed=5):
    """1 + limbs * per node positions: a centre and straight limbs of length 0.5 (a tree with a junction whatever the motion)."""
    g = torch.Generator().manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.tensor([[0.0, 1.0, 0.2], [0.9, -0.4, 0.0], [-0.8, -0.5, 0.3], [0.1, 0.2, -1.0]])[:limbs], dim=-1)
    s = torch.arange(1, per + 1) / per * 0.5
    pts = (dirs[:, None, :] * s[None, :, None]).reshape(-1, 3) + 0.002 * torch.randn(limbs * per, 3, generator=g)
    return torch.cat([torch.zeros(1, 3), pts])


class BendingNodeNet(torch.nn.Module):
    """A smooth closed-form node network: a shear that grows with time plus a bend that grows with the distance from the centre
    (limbs stay chains a few straight bones can follow); the other attributes follow d_xyz."""

    def __init__(self):
        super().__init__()
        self.B = torch.nn.Parameter(torch.tensor([[0.10, 0.30, -0.05], [-0.25, 0.05, 0.10], [0.05, -0.10, 0.08]]))
        self.v = torch.nn.Parameter(torch.tensor([0.6, -0.4, 0.9]))

    def forward(self, x, t, **kwargs):
        d = torch.sin(3.0 * t) * (x @ self.B) + torch.sin(2.0 * t + 0.5) * (x * x).sum(-1, keepdim=True) * 4.0 * self.v
        z4 = torch.zeros(x.shape[0], 4, dtype=d.dtype, device=d.device)
        return {"d_xyz": d, "d_rotation": z4 + 0.01 * d[:, :1], "d_scaling": 0.1 * d, "local_rotation": z4.clone(), "hidden": None,
                "d_opacity": None, "d_color": None}


def stage1_scene(device="cuda", M=64, N=500, hyper=2, seed=9):
    """A small trained-stage-1 stand-in: a ``ControlNodeWarp`` of M nodes on the star above with the node network above, and a ``GaussianModel`` of N Gaussians scattered around the nodes.  ``(warp, gaussians)``."""
    from riggs_amd.control_nodes import ControlNodeWarp
    from riggs_amd.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(seed)
    nodes = star_nodes(3, (M - 1) // 3)
    assert nodes.shape[0] == M
    warp = ControlNodeWarp(node_num=M, K=3, hyper_dim=hyper, with_node_weight=True, network=BendingNodeNet()).to(device)
    warp.nodes.data = torch.cat([nodes, 1e-2 * torch.ones(M, hyper)], -1).to(device)
    warp._node_radius.data = (torch.log(torch.tensor(0.05)) + 0.3 * torch.rand(M, generator=g)).to(device)
    warp._node_weight.data = torch.zeros(M, 1, device=device)
    xyz = nodes[torch.randint(0, M, (N,), generator=g)] + 0.02 * torch.randn(N, 3, generator=g)
    gm = GaussianModel.from_tensors(xyz, torch.rand(N, 1, 3, generator=g), torch.zeros(N, 15, 3), torch.full((N, 3), -4.0),
                                    torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(N, 1), torch.zeros(N, 1), device=device)
    gm.feature = (0.01 * torch.randn(N, hyper, generator=g)).to(device)
    return warp, gm
