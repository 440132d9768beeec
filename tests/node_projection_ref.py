"""float64 reference of the stage-1 node projection term (/root/reference/train_gui.py:1134-1138), restated in torch:
``project_nodes_to_2d_elements`` (utils/other_utils.py:101-127; elements are (row, col), ``K``'s principal point when the camera
has one) and ``pytorch3d.loss.chamfer_distance(x[None], y[None], norm=1)`` with its default reductions (pytorch3d is not
installed, as for oracle/loss_ref.py: mean of the nearest L1 distances over the points of each side, the two sides summed).
The projection is pinned against the reference's own by tests/golden/nodeproj_*.npz."""
import math

import numpy as np
import torch


def intrinsics(FoVx, FoVy, H, W, K=None):
    fy = H / (2 * math.tan(FoVy * 0.5))
    fx = W / (2 * math.tan(FoVx * 0.5))
    if K is not None and np.size(K):
        return fx, fy, float(K[0][2]), float(K[1][2])
    return fx, fy, W / 2, H / 2


def project(nodes, view, fx, fy, cx, cy):
    """(M, 2) elements (row, col) of (M, 3) ``nodes``; ``view`` is world_view_transform (row-vector convention)."""
    tr = nodes @ view[:3, :3] + view[3, :3]
    return torch.stack([fy * tr[:, 1] / tr[:, 2] + cy, fx * tr[:, 0] / tr[:, 2] + cx], -1)


def chamfer_l1(x, y):
    d = (x[:, None, :] - y[None, :, :]).abs().sum(-1)
    return d.min(1).values.mean() + d.min(0).values.mean()


def node_projection_loss(nodes, view, fx, fy, cx, cy, thinned, pixel_count=None):
    """(loss, dloss/dnodes) in float64 from numpy inputs."""
    x = torch.from_numpy(np.asarray(nodes, np.float64)).requires_grad_(True)
    V = torch.from_numpy(np.asarray(view, np.float64))
    y = torch.from_numpy(np.asarray(thinned, np.float64))
    if pixel_count is not None:
        y = y[:int(pixel_count)]
    loss = chamfer_l1(project(x, V, fx, fy, cx, cy), y)
    loss.backward()
    return float(loss.detach()), x.grad.numpy()
