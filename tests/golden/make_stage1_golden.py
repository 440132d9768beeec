"""Stage-1 fixtures for the node regularisers and ControlNodeWarp's trainer surface, from the reference Python on CPU
(tests/golden/_ref_shim.py).  ``pytorch3d.ops.knn_points`` is restated with its published contract and a stable tie order
(the lowest index first), as the HIP kernel computes it.

  stage1_arap_m64_t3.npz   (a) cal_connectivity_from_points (mode 'nn', K = 10) + cal_arap_error at M = 64, T = 3: some
                           edges beyond the radius, one node whose edges keep a coordinate unchanged; value and gradient
  stage1_arap_m600_t3.npz  (b) the same at M = 600, with the np.random.choice rows cal_arap_error drew
  stage1_losses_m300.npz   (c) ControlNodeWarp (hyper 8, node weights, a closed-form node network with parameters):
                           arap_loss, elastic_loss, acc_loss, the time inputs the network saw, and each loss's gradients to
                           the network parameters, nodes, _node_radius and _node_weight
  stage1_densify_m64.npz   (d) init (recorded farthest-point start), cal_node_importance, one Adam step, densify(force_dp):
                           node parameters, exp_avg / exp_avg_sq of the 'nodes' group, the node Gaussians' rows
  stage1_surface.json      (e) the ControlNodeWarp members train_gui.py and scene/deform_model.py touch
"""
import collections
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim as S  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.node_reg_ref import ClosedFormNodeNet, DensifyOpt, TimeReplay, densify_inputs, densify_step_loss  # noqa: E402

SURFACE = ["name", "init", "inited", "as_gaussians", "init_gaussians", "query_network", "use_hash", "elastic_loss", "acc_loss",
           "arap_loss", "forward", "reg_loss", "densify", "cal_node_importance", "state_dict", "load_state_dict", "param_names",
           "update", "cal_nn_weight", "nodes_color_visualization", "cached_nn_weight", "nn_weight", "nn_dist", "nn_idxs",
           "trainable_parameters", "node_deform", "nodes", "_node_radius", "_node_weight", "node_num", "hyper_dim", "K",
           "skinning", "enable_dp", "lambda_arap_landmarks", "lambda_arap_steps", "network", "expand_time"]


def np_(t):
    return t.detach().cpu().numpy().astype(np.float32)


_KNN = collections.namedtuple("KNN", ["dists", "idx", "knn"])


def knn_points_stable(p1, p2, lengths1=None, lengths2=None, K=1, **kw):
    d = torch.zeros(p1.shape[1], p2.shape[1])
    for c in range(p1.shape[2]):
        t = p1[0][:, None, c] - p2[0][None, :, c]
        d = d + t * t
    dist, idx = torch.sort(d, dim=1, stable=True)
    return _KNN(dist[None, :, :K].contiguous(), idx[None, :, :K].contiguous(), None)


def _install():
    S.install()
    import pytorch3d.ops as p3o
    import pytorch3d as p3
    p3o.knn_points = knn_points_stable
    p3.ops = p3o


def fixture_arap(name, seed, M, T):
    with S.quiet():
        from utils import deform_utils as DU
    DU.pytorch3d.ops.knn_points = knn_points_stable
    g = torch.Generator().manual_seed(seed)
    side = 0.35 * (M / 64) ** (1 / 3)
    p0 = torch.rand(M, 3, generator=g) * side
    seq = torch.stack([p0] + [p0 + 0.02 * torch.randn(M, 3, generator=g) for _ in range(T - 1)])
    seq[1:, 5, 0] = seq[0, 5, 0]  # node 5 keeps its x coordinate ...
    ii, jj, nn, weight = DU.cal_connectivity_from_points(seq[0], K=10)
    idx = -torch.ones(M, 10, dtype=torch.long)
    idx[ii, nn] = jj
    # ... and so do its neighbours in x: every edge of row 5 keeps its x component
    nb = idx[5][idx[5] >= 0]
    seq[1:, nb, 0] = seq[0, nb, 0]
    ii, jj, nn, weight = DU.cal_connectivity_from_points(seq[0], K=10)
    drawn = []
    choice = np.random.choice

    def rec_choice(*a, **k):
        r = choice(*a, **k)
        drawn.append(np.asarray(r).copy())
        return r
    np.random.choice = rec_choice
    try:
        s = seq.clone().requires_grad_(True)
        e = DU.cal_arap_error(s, ii, jj, nn)
        e.backward()
    finally:
        np.random.choice = choice
    rows = drawn[0].astype(np.int32) if drawn else np.arange(M, dtype=np.int32)
    z = dict(seq=np_(seq), ii=ii.numpy(), jj=jj.numpy(), nn=nn.numpy(), weight=np_(weight), arap=np.float32(e.item()),
             grad_seq=np_(s.grad), rows=rows)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **z)
    print("wrote", name, "edges", ii.shape[0], "of", M * 10, "rows", rows.shape[0], "energy", e.item())


def _ref_warp(M, seed, **kw):
    with S.quiet():
        from utils.time_utils import ControlNodeWarp
        cn = ControlNodeWarp(is_blender=True, node_num=M, K=3, hyper_dim=8, with_node_weight=True, is_scene_static=True, **kw)
    cn.network = TimeReplay(ClosedFormNodeNet())
    g = torch.Generator().manual_seed(seed)
    cn.nodes = torch.nn.Parameter(torch.cat([torch.rand(M, 3, generator=g) * 0.5, 1e-2 + 0.02 * torch.randn(M, 8, generator=g)], -1))
    cn._node_radius = torch.nn.Parameter(np.log(0.15) + 0.3 * torch.randn(M, generator=g))
    cn._node_weight = torch.nn.Parameter(0.5 * torch.randn(M, 1, generator=g))
    return cn


LOSS_CALLS = {"arap": dict(delta_t=0.5, t_samp_num=3), "elastic": dict(t=0.4, delta_t=0.05), "acc": dict(t=0.4, delta_t=0.1)}


def fixture_losses(name, seed, M):
    cn = _ref_warp(M, seed)
    cn.train()
    z = dict(nodes=np_(cn.nodes), _node_radius=np_(cn._node_radius), _node_weight=np_(cn._node_weight))
    for k, v in cn.network.net.named_parameters():
        z["net_" + k] = np_(v)
    for loss, kw in LOSS_CALLS.items():
        kw = {a: (torch.tensor(b) if a == "t" else b) for a, b in kw.items()}
        cn.zero_grad(set_to_none=True)
        cn.network.seen = []
        v = getattr(cn, loss + "_loss")(**kw)
        v.backward()
        z[loss] = np.float32(v.item())
        z[loss + "_t"] = np.stack([np_(t).reshape(-1) for t in cn.network.seen])
        for k, p in list(cn.network.net.named_parameters()) + [("nodes", cn.nodes), ("_node_radius", cn._node_radius),
                                                              ("_node_weight", cn._node_weight)]:
            z[loss + "_grad_" + k] = np_(p.grad) if p.grad is not None else np.zeros(p.shape, np.float32)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **z)
    print("wrote", name, {k: float(z[k]) for k in LOSS_CALLS})


def fixture_densify(name, seed, M):
    from utils import time_utils as TU
    fps = TU.farthest_point_sample
    starts = []

    def fps_rec(xyz, npoint):
        st = torch.get_rng_state()
        starts.append(int(torch.randint(0, xyz.shape[1], (xyz.shape[0],), dtype=torch.long)[0]))
        torch.set_rng_state(st)
        return fps(xyz, npoint)
    TU.farthest_point_sample = fps_rec
    cn = _ref_warp(M, seed, enable_densify_prune=True)
    x, pcl, feature, x_grad = densify_inputs(seed)
    with S.quiet():
        init_idx = cn.init(DensifyOpt(), pcl)
    TU.farthest_point_sample = fps
    opt = torch.optim.Adam(cn.trainable_parameters(), lr=1e-3, eps=1e-15)
    densify_step_loss(cn).backward()
    opt.step()
    imp, avg_x, cnt = cn.cal_node_importance(x=x, K=3, weights=x_grad.norm(dim=-1), feature=feature)
    with S.quiet():
        cn.densify(max_grad=0.02, optimizer=opt, x=x, x_grad=x_grad.clone(), feature=feature, force_dp=True)
    z = dict(fps_start=np.int64(starts[0]), init_idx=init_idx.numpy(), importance=np_(imp), avg_x=np_(avg_x), edge_count=np_(cnt),
             nodes=np_(cn.nodes), _node_radius=np_(cn._node_radius), _node_weight=np_(cn._node_weight),
             color=np_(cn.nodes_color_visualization))
    grp = [g_ for g_ in opt.param_groups if g_["name"] == "nodes"][0]
    for k, p in zip(cn.param_names, grp["params"]):
        z["exp_avg_" + k] = np_(opt.state[p]["exp_avg"])
        z["exp_avg_sq_" + k] = np_(opt.state[p]["exp_avg_sq"])
    for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        z["gs" + k] = np_(getattr(cn.as_gaussians, k))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **z)
    print("wrote", name, "start", starts[0], "nodes", M, "->", cn.nodes.shape[0], "selected", int((imp > 0.02).sum()),
          "unused", int((cnt == 0).sum()))


def surface(path):
    with S.quiet():
        from utils.time_utils import ControlNodeWarp
        cn = ControlNodeWarp(is_blender=True, node_num=16, K=3, hyper_dim=8, is_scene_static=True, with_arap_loss=True)
    names = [n for n in SURFACE if hasattr(type(cn), n) or hasattr(cn, n)]
    with open(path, "w") as f:
        json.dump(names, f, indent=1)
    print("wrote", path, len(names), "names")


if __name__ == "__main__":
    _install()
    torch.manual_seed(0)
    fixture_arap("stage1_arap_m64_t3", 5, 64, 3)
    np.random.seed(600)
    fixture_arap("stage1_arap_m600_t3", 6, 600, 3)
    torch.manual_seed(1)
    fixture_losses("stage1_losses_m300", 7, 300)
    torch.manual_seed(2)
    fixture_densify("stage1_densify_m64", 8, 64)
    surface(os.path.join(HERE, "stage1_surface.json"))
