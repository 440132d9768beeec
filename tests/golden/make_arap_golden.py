"""Record the reference's own ARAP drag (utils/arap_deform.py: ARAPDeformer.deform, lap_deform.py: LapDeform.deform_arap) through
the import shim — run in the build container only:   python tests/golden/make_arap_golden.py

Emits tests/golden/arap_*.npz: inputs, the reference's ``weight`` and padded ``nn`` lists, positions and quaternions of
``deform(return_R=True)``, and the positions and quaternions after each further call chained through ``init_verts`` (the reference's
NUM_ITER is a local constant: a chained call is three more rounds from where the last one stopped).

A CONDITION, asserted here: no fixture has a dropped edge or a non-finite weight.  The reference's weights are NaN as soon as one
edge is dropped (its mean distance is inf), so only such inputs are the reference's own word: compact clouds under an explicit large
radius at small N, and the trajectory mode for LapDeform (whose distances are T times smaller against the same radius).

pytorch3d is not installed: ``knn_points`` is make_golden.py's stand-in for its published contract (K nearest by squared distance,
ascending), wrapped so that ``.dists`` / ``.idx`` exist.  The reference Python itself is never copied; fixtures are data.
"""
import collections
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim as S  # noqa: E402

S.install()

KNN = collections.namedtuple("KNN", "dists idx knn")


def knn_points_published(p1, p2, lengths1=None, lengths2=None, K=1, **kw):
    d = ((p1[0][:, None, :] - p2[0][None, :, :]) ** 2).sum(-1)
    dist, idx = d.topk(K, dim=1, largest=False, sorted=True)
    return KNN(dist[None], idx[None], None)


import pytorch3d  # noqa: E402  (the shim's stub modules)
import pytorch3d.ops as p3o  # noqa: E402
p3o.knn_points = knn_points_published
pytorch3d.ops = p3o
with S.quiet():
    from utils.arap_deform import ARAPDeformer  # noqa: E402
    from lap_deform import LapDeform  # noqa: E402


def np_(t):
    return t.detach().cpu().numpy()


def padded_lists(d):
    nn = torch.full((d.N, d.K), -1, dtype=torch.int32)
    nn[d.ii, d.nn] = d.jj.to(torch.int32)
    return nn


def record(name, tool, deformer, verts, handles, handle_pos, chain, **extra):
    """``tool``: what is called (ARAPDeformer.deform or LapDeform.deform_arap); ``deformer``: the ARAPDeformer behind it."""
    nn = padded_lists(deformer)
    weight = deformer.weight.detach()
    assert bool((nn >= 0).all()), "%s: the reference dropped an edge: its weights are not its word there" % name
    assert bool(torch.isfinite(weight).all()), "%s: non-finite weight" % name
    pos, quat = [], []
    init = None
    with torch.no_grad(), S.quiet():
        for _ in range(chain):
            p, q, _s = tool(handles, handle_pos, init_verts=init, return_R=True)
            assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(q).all()), name
            pos.append(np_(p))
            quat.append(np_(q))
            init = p.clone()
    out = dict(verts=np_(verts), handle_idx=np.asarray(handles, np.int32), handle_pos=np.asarray(handle_pos, np.float32),
               K=np.int32(deformer.K), radius=np.float32(float(deformer.radius)), weight=np_(weight), nn=np_(nn),
               pos=np.stack(pos), quat=np.stack(quat), **extra)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, "N", deformer.N, "K", deformer.K, "handles", list(handles), "moved by",
          float(np.abs(pos[0] - np_(verts)).max()))


def fixture_deformer(name, seed, N, M, K, radius, chain=3):
    g = torch.Generator().manual_seed(seed)
    verts = torch.rand(N, 3, generator=g) - 0.5
    handles = torch.randperm(N, generator=g)[:M]
    handle_pos = verts[handles] + 0.25 * torch.randn(M, 3, generator=g)
    with S.quiet():
        d = ARAPDeformer(verts.clone(), K=K, radius=radius)
    record(name, lambda h, p, **kw: d.deform(torch.as_tensor(h).long(), torch.as_tensor(p).float(), **kw), d, verts,
           handles.tolist(), handle_pos.numpy(), chain)


def fixture_lapdeform(name, seed, N, M, T=16, chain=2):
    """The editor's construction (train_gui.py:204-223): LapDeform over the nodes at one time with their T-sample trajectory."""
    g = torch.Generator().manual_seed(seed)
    verts = torch.rand(N, 3, generator=g) - 0.5
    t = torch.linspace(0, 1, T)[None, :, None]
    sway = 0.1 * torch.randn(N, 1, 3, generator=g) * torch.sin(3.0 * t) + 0.05 * torch.randn(1, 1, 3, generator=g) * t
    trajectory = verts[:, None] + sway
    handles = torch.randperm(N, generator=g)[:M]
    handle_pos = verts[handles] + 0.2 * torch.randn(M, 3, generator=g)
    with S.quiet():
        tool = LapDeform(init_pcl=verts.clone(), K=4, trajectory=trajectory, node_radius=torch.full((N,), 0.1))
    record(name, tool.deform_arap, tool.arap_deformer, verts, handles.tolist(), handle_pos.numpy(), chain, trajectory=np_(trajectory))


if __name__ == "__main__":
    fixture_deformer("arap_n20_m1_k10", 1, N=20, M=1, K=10, radius=10.0)
    fixture_deformer("arap_n40_m2_k4", 2, N=40, M=2, K=4, radius=10.0)
    fixture_lapdeform("arap_lap_n65_m3_traj", 3, N=65, M=3)
