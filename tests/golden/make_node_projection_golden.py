"""Golden vectors of the stage-1 node projection term (train_gui.py:1133-1139) from the REAL RigGS reference (CPU) — run in the
build container only:   python tests/golden/make_node_projection_golden.py

The projection is the reference's own ``project_nodes_to_2d_elements`` (utils/other_utils.py:101-127) on a reference ``Camera``;
``pytorch3d.loss.chamfer_distance(x, y, norm=1)`` is not installed and is restated from its published definition (default
reductions: mean over the points of each side, the two sides summed), as for skelproj_*.npz.  Only data is written:
nodeproj_m512_p700.npz (no intrinsic matrix: the principal point is the image centre) and nodeproj_m33_p90_K.npz (with ``K``).
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim as S  # noqa: E402

S.install()
with S.quiet():
    from scene.cameras import Camera  # noqa: E402
    from utils.other_utils import project_nodes_to_2d_elements  # noqa: E402


def chamfer_l1_published(x, y):
    """pytorch3d.loss.chamfer_distance(x[None], y[None], norm=1)[0] by its published definition."""
    d = (x[:, None, :] - y[None, :, :]).abs().sum(-1)
    return d.min(1).values.mean() + d.min(0).values.mean()


def fixture(name, seed, M, P, from_K):
    g = torch.Generator().manual_seed(seed)
    nodes = (0.6 * (torch.rand(M, 3, generator=g) - 0.5) * torch.tensor([1.0, 1.6, 1.0])).requires_grad_(True)
    az, el, rad = math.radians(-20.0), math.radians(10.0), 3.0
    eye = np.array([rad * math.cos(el) * math.sin(az), -rad * math.sin(el), -rad * math.cos(el) * math.cos(az)])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(np.array([0.0, -1.0, 0.0]), fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    Rc2w = np.stack([right, up, fwd], axis=1)
    T = -Rc2w.T @ eye
    H, W = 135, 180
    fovx = 0.6911112
    K = None
    if from_K:
        fx = W / (2 * math.tan(fovx / 2))
        K = np.array([[fx, 0, W / 2 - 4.25], [0, fx, H / 2 + 6.5], [0, 0, 1]], dtype=np.float64)
    cam = Camera(0, Rc2w, T, fovx, fovx * 0.8, torch.zeros(3, H, W), None, "c", 0, data_device="cpu", fid=0.5, K=K)
    with torch.no_grad():
        proj0 = project_nodes_to_2d_elements(cam, nodes.detach())
    # thinned silhouette pixels (row, col): near the projected nodes, jittered, some far outliers, one exact repeat
    pick = torch.randint(0, M, (P,), generator=g)
    thinned = (proj0[pick] + 5.0 * torch.randn(P, 2, generator=g)).round()
    thinned[: P // 10] = torch.stack([torch.randint(0, H, (P // 10,), generator=g),
                                      torch.randint(0, W, (P // 10,), generator=g)], -1).float()
    thinned[-1] = thinned[0]
    proj = project_nodes_to_2d_elements(cam, nodes)
    loss = chamfer_l1_published(proj, thinned)
    loss.backward()
    out = dict(d_nodes=nodes.detach().numpy(), world_view_transform=cam.world_view_transform.detach().numpy(), FoVx=cam.FoVx,
               FoVy=cam.FoVy, image_height=H, image_width=W, K=(np.zeros((0, 0)) if K is None else np.asarray(K)),
               thinned=thinned.numpy(), projected=proj.detach().numpy(), loss=float(loss.detach()),
               grad_nodes=nodes.grad.numpy())
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, "nodes", M, "pixels", P, "loss", out["loss"])


if __name__ == "__main__":
    fixture("nodeproj_m512_p700", 81, 512, 700, False)
    fixture("nodeproj_m33_p90_K", 82, 33, 90, True)
