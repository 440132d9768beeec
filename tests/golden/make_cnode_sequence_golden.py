"""Goldens for ``ControlNodeWarp.deform_sequence`` from the REAL RigGS reference (CPU) — run in the build container only:
    python tests/golden/make_cnode_sequence_golden.py

The reference has no sequence call: its ``ControlNodeWarp.forward`` (utils/time_utils.py:1133-1236) is called once per frame,
every node attribute of the frame handed over through its own ``animation_d_values`` hook (:1141-1144), and the frames are
stacked.  Emits tests/golden/cnodeseq_*.npz (inputs + expected outputs); the reference's Python is never copied.

A fixture is kept only if, for every Gaussian, the K-th and the (K+1)-th nearest node differ by more than 1e-5 relative in
squared distance (another seed is taken otherwise): float32 and float64 then select the same K nodes, so ``nn_idx`` is
compared exactly on every row."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import S, knn_points_published, np_  # noqa: E402

TIE_GAP = 1e-5
ATTRS = (("d_xyz", 3, 0.1), ("d_rotation", 4, 0.2), ("d_scaling", 3, 0.05), ("local_rotation", 4, 0.3), ("d_opacity", 1, 0.3),
         ("d_color", 3, 0.2))


def tie_gap(x, feature, nodes, K, hyper):
    """min over the rows of (d_{K+1} - d_K) / d_{K+1} in float64."""
    xa = np.concatenate([x, feature[:, :hyper]], -1).astype(np.float64) if hyper > 0 else x.astype(np.float64)
    na = nodes[:, :3 + hyper].astype(np.float64)
    d = np.sort(((xa[:, None] - na[None]) ** 2).sum(-1), axis=1)
    return float(((d[:, K] - d[:, K - 1]) / d[:, K]).min())


def fixture(name, seed, N, M, T, K, hyper, local_frame, d_rot_as_res, pred):
    import pytorch3d.ops as p3o
    import pytorch3d as p3
    p3o.knn_points = knn_points_published
    p3.ops = p3o
    with S.quiet():
        from utils.time_utils import ControlNodeWarp
    while True:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(N, 3, generator=g) * 0.5
        pick = torch.randint(0, N, (M,), generator=g)
        nodes = torch.cat([x[pick] + 0.05 * torch.randn(M, 3, generator=g), 1e-2 + 0.02 * torch.randn(M, hyper, generator=g)], -1)
        feature = 0.02 * torch.randn(N, hyper + 1, generator=g) if hyper > 0 else None
        gap = tie_gap(np_(x), np_(feature) if feature is not None else None, np_(nodes), K, hyper)
        if gap > TIE_GAP:
            break
        print(name, "seed", seed, "has a near-tie (gap %.3g): next seed" % gap)
        seed += 1
    with S.quiet():
        cn = ControlNodeWarp(is_blender=True, node_num=M, K=K, with_node_weight=True, local_frame=local_frame,
                             d_rot_as_res=d_rot_as_res, hyper_dim=hyper, is_scene_static=True, pred_opacity=pred, pred_color=pred)
    cn.nodes = torch.nn.Parameter(nodes)
    cn._node_radius = torch.nn.Parameter(math.log(0.15) + 0.3 * torch.randn(M, generator=g))
    cn._node_weight = torch.nn.Parameter(0.5 * torch.randn(M, 1, generator=g))
    mask = torch.rand(N, 1, generator=g)
    times = torch.linspace(0, 1, T)
    attrs = {k: s * torch.randn(T, M, c, generator=g) for k, c, s in ATTRS}
    keys = ["d_xyz", "d_rotation", "d_scaling", "d_nodes"] + (["d_opacity", "d_color"] if pred else [])
    outs = {k: [] for k in keys}
    cn.eval()
    with torch.no_grad():
        for f in range(T):
            out = cn(x, times[f], feature, mask, animation_d_values={k: v[f] for k, v in attrs.items()})
            for k in keys:
                outs[k].append(np_(out[k]))
        nn_weight, nn_dist, nn_idx = cn.cal_nn_weight(x=x, feature=feature)
    z = dict(x=np_(x), nodes=np_(nodes), _node_radius=np_(cn._node_radius), _node_weight=np_(cn._node_weight),
             feature=(np_(feature) if feature is not None else np.zeros((0, 0), np.float32)), motion_mask=np_(mask), times=np_(times),
             K=K, hyper_dim=hyper, local_frame=local_frame, d_rot_as_res=d_rot_as_res, pred=pred, seed=seed, tie_gap=gap,
             nn_idx=nn_idx.numpy().astype(np.int32), nn_weight=np_(nn_weight), nn_dist=np_(nn_dist))
    for k, v in attrs.items():
        z["attr_" + k] = np_(v)
    for k in keys:
        z["out_" + k] = np.stack(outs[k])
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **z)
    print("wrote", name, "seed", seed, "tie gap %.3g" % gap, {k: z["out_" + k].shape for k in keys})


if __name__ == "__main__":
    fixture("cnodeseq_local_res_h8", 4101, N=300, M=48, T=4, K=3, hyper=8, local_frame=True, d_rot_as_res=True, pred=False)
    fixture("cnodeseq_abs_h0_pred", 4102, N=300, M=48, T=4, K=3, hyper=0, local_frame=False, d_rot_as_res=False, pred=True)
