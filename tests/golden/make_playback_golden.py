"""Golden vectors for pose-track playback, captured from the REAL RigGS reference (CPU) — run in the build container only:
    python tests/golden/make_playback_golden.py
Never imported by a test.  The reference's own slerp_batch / run_interpolation (skeleton_utils/interpolation_utils.py),
get_geometric_color / get_color_for_skinning_weights (skeleton_utils/visualization.py) and SkeletonWarp.deform_by_pose run here;
the files hold their inputs and results only."""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import S, make_warp, np_, random_tree  # noqa: E402

try:
    import matplotlib  # noqa: F401  (visualization.py imports its colour maps; nothing used here touches them)
except ImportError:
    mpl = types.ModuleType("matplotlib")
    mpl.cm = types.ModuleType("matplotlib.cm")
    sys.modules["matplotlib"], sys.modules["matplotlib.cm"] = mpl, mpl.cm
with S.quiet():
    from skeleton_utils.interpolation_utils import run_interpolation, slerp_batch  # noqa: E402
    from skeleton_utils.visualization import get_color_for_skinning_weights, get_geometric_color  # noqa: E402


def save(name, **kw):
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **kw)
    print("wrote", name, {k: np.asarray(v).shape for k, v in kw.items()})


def fixture_slerp(name, seed, n, t):
    """Random un-normalised pairs; row 0 a pair with a negative dot product, row 1 an identical pair q1 = 2 q0 (the linear branch,
    through 0 / 0), row 2 an antipodal pair q1 = -q0."""
    g = torch.Generator().manual_seed(seed)
    q0 = torch.randn(n, 4, generator=g) * (0.5 + torch.rand(n, 1, generator=g))
    q1 = torch.randn(n, 4, generator=g) * (0.5 + torch.rand(n, 1, generator=g))
    if float((q0[0] * q1[0]).sum()) > 0:
        q1[0] = -q1[0]
    q1[1] = 2.0 * q0[1]
    q1[2] = -q0[2]
    out = slerp_batch(q0, q1, t)
    assert bool(torch.isfinite(out).all()) and float((q0[0] * q1[0]).sum()) < 0
    save(name, q0=np_(q0), q1=np_(q1), t=np_(t), out=np_(out))


def key_poses(g, P, J, key="local_rotation2", spread=0.4):
    return [{key: torch.tensor([1.0, 0, 0, 0]) + spread * torch.randn(J, 4, generator=g),  # NOT normalised
             "global_trans": 0.05 * torch.randn(1, 3, generator=g)} for _ in range(P)]


def fixture_interp(name, seed, P, J, num_frames):
    g = torch.Generator().manual_seed(seed)
    keys = key_poses(g, P, J)
    with S.quiet():
        out = run_interpolation(keys, "cpu", num_frames=num_frames)
    save(name, key_rot=np_(torch.stack([k["local_rotation2"] for k in keys])),
         key_trans=np_(torch.stack([k["global_trans"] for k in keys])), num_frames=np.int64(num_frames),
         local_rotation=np_(out["local_rotation2"]), global_trans=np_(out["global_trans"]), num=np.int64(out["num"]))


def cloud(g, joints, parents, N):
    J = joints.shape[0]
    bone = torch.randint(1, J, (N,), generator=g)
    t = torch.rand(N, 1, generator=g) * 1.4 - 0.2
    a, b = joints[parents[bone]], joints[bone]
    return a + t * (b - a) + 0.06 * torch.randn(N, 3, generator=g)


def fixture_colors(name, seed, J, N, K):
    g = torch.Generator().manual_seed(seed)
    joints, parents = random_tree(g, J)
    sw = make_warp(joints, parents, K)
    rho = math.log(0.15) + 0.3 * torch.randn(J, generator=g)
    sw._node_radius.data = rho.clone()
    x = cloud(g, joints, parents, N)
    w, d2, idx = sw.cal_nn_weight_skeleton(x=x, nodes=sw.nodes)
    nodes = sw.nodes.detach()[:, :3]
    save(name, joints=np_(joints), parents=np_(parents), node_radius_log=np_(rho), x=np_(x), K=np.int64(K), nn_idx=np_(idx),
         nn_weight=np_(w), node_colors=np_(get_geometric_color(nodes)), point_colors=np_(get_geometric_color(x)),
         colors=np_(get_color_for_skinning_weights(x, vn_idx=idx, vn_weight=w, control_points=nodes)))


def fixture_sequence(name, seed, J, N, K, num_frames, chain=False, mask_random=False):
    g = torch.Generator().manual_seed(seed)
    joints, parents = random_tree(g, J, chain)
    sw = make_warp(joints, parents, K)
    rho = math.log(0.15) + 0.3 * torch.randn(J, generator=g)
    sw._node_radius.data = rho.clone()
    x = cloud(g, joints, parents, N)
    mask = torch.sigmoid(torch.randn(N, 1, generator=g)) if mask_random else torch.ones(N, 1)
    keys = key_poses(g, 2, J, spread=0.3)
    with S.quiet():
        track = run_interpolation(keys, "cpu", num_frames=num_frames)
    outs = []
    with torch.no_grad():
        for f in range(track["num"]):
            outs.append(sw.deform_by_pose(x, {"local_rotation": track["local_rotation2"][f], "global_trans": track["global_trans"][f]}, mask))
    save(name, joints=np_(joints), parents=np_(parents), node_radius_log=np_(rho), x=np_(x), motion_mask=np_(mask), K=np.int64(K),
         key_rot=np_(torch.stack([k["local_rotation2"] for k in keys])), key_trans=np_(torch.stack([k["global_trans"] for k in keys])),
         num_frames=np.int64(num_frames), local_rotation=np_(track["local_rotation2"]), global_trans=np_(track["global_trans"]),
         d_xyz=np_(torch.stack([o["d_xyz"] for o in outs])), d_rotation=np_(torch.stack([o["d_rotation"] for o in outs])),
         d_nodes=np_(torch.stack([o["d_nodes"] for o in outs])))


if __name__ == "__main__":
    fixture_slerp("playback_slerp_n19_m20", 301, 19, torch.linspace(0, 1, steps=21)[:-1])
    fixture_slerp("playback_slerp_n7_m1", 302, 7, torch.tensor([0.37]))
    fixture_interp("playback_interp_p3_j24_f7", 303, 3, 24, 7)
    fixture_colors("playback_colors_tree24_n300", 304, 24, 300, -1)
    fixture_colors("playback_colors_tree24_n300_k3", 305, 24, 300, 3)
    fixture_sequence("playback_seq_tree24_n300_m5", 306, 24, 300, -1, 5, mask_random=True)
    fixture_sequence("playback_seq_chain8_n257_m3_k3", 307, 8, 257, 3, 3, chain=True)
