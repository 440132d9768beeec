"""The oracle of the control-node sequence blend (TEST INFRASTRUCTURE ONLY): ``oracle.cnode_ref.forward`` — float64 — looped
over the frames of (T, M, c) node attributes and stacked frame-major.  ``nn_idx``: a kernel's own neighbour lists (the float64
selection rule admits them where ``tests.cnode_f64_ref.selection_violations`` is 0), as tests/test_gpu_cnode.py:96 takes them;
None: the oracle's own K smallest distances.  The lists and weights do not depend on the frame: they are returned once."""
import os

import numpy as np

from oracle import cnode_ref as O

OUTS = ("d_xyz", "d_rotation", "d_scaling", "d_nodes")
GOLDENS = ("cnodeseq_local_res_h8", "cnodeseq_abs_h0_pred")
TIE_GAP = 1e-5  # the makers' condition: (d_{K+1} - d_K) / d_{K+1} of every row exceeds it


def forward_sequence(x, feature, mask, nodes, node_radius_log, node_weight_logit, attrs, K, hyper_dim, local_frame, d_rot_as_res,
                     nn_idx=None):
    T = np.asarray(attrs["d_xyz"]).shape[0]
    N, M = np.asarray(x).shape[0], np.asarray(nodes).shape[0]
    out = {"d_xyz": np.zeros((T, N, 3)), "d_rotation": np.zeros((T, N, 4)), "d_scaling": np.zeros((T, N, 3)), "d_nodes": np.zeros((T, M, 3))}
    for f in range(T):
        r = O.forward(x, feature, mask, nodes, node_radius_log, node_weight_logit, {k: np.asarray(v)[f] for k, v in attrs.items()},
                      K=K, hyper_dim=hyper_dim, local_frame=local_frame, d_rot_as_res=d_rot_as_res, nn_idx=nn_idx)
        for k in OUTS:
            out[k][f] = r[k]
        if f == 0:
            out.update(nn_weight=r["nn_weight"], nn_dist=r["nn_dist"], nn_idx=r["nn_idx"])
    if T == 0:
        w, dist, idx = O.cal_nn_weight(x, feature, nodes, node_radius_log, node_weight_logit, K, hyper_dim, nn_idx)
        out.update(nn_weight=w, nn_dist=dist, nn_idx=idx)
    return out


def golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


def tie_gap(z):
    """min over the rows of (d_{K+1} - d_K) / d_{K+1}, float64, of a golden's cloud."""
    K, h = int(z["K"]), int(z["hyper_dim"])
    xa = z["x"].astype(np.float64)
    if h > 0:
        xa = np.concatenate([xa, z["feature"][:, :h].astype(np.float64)], -1)
    na = z["nodes"][:, :3 + h].astype(np.float64)
    d = np.sort(((xa[:, None] - na[None]) ** 2).sum(-1), axis=1)
    return float(((d[:, K] - d[:, K - 1]) / d[:, K]).min())
