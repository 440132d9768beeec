"""Golden vectors of the stage-2 skeleton extraction and of farthest-point sampling from the REAL RigGS reference (CPU) — run in
the build container only:   python tests/golden/make_skeleton_init_golden.py

Skeleton fixtures (skelinit_per{12,30,60,100}.npz, and skelinit_per30_twigs.npz with short side branches on the limbs): a figure of one node at the origin and five straight limbs of ``per`` nodes
each, moving over F frames (every limb swings about the origin, its outer half also about the limb's midpoint; sinusoidal angles
with a phase per limb).  The reference's ``obtain_skeleton_tree`` (skeleton_utils/extract_skeleton_utils.py:426-471) is run whole
and stage by stage (``gene_tree``, ``adjust_arrow_dir``, ``prune_tree``, ``simplify_tree``, ``adjust_arrow_dir``); the fixture holds
the inputs, the sampling start (seed, then ``centroids[0, 0]``), the sampled indices, ``mean_distances`` and every stage's output.  A fixture is written
only if tree and indices stay the same with all inputs scaled by 1 + 1e-5 and by 1 - 1e-5.  To keep each file under 100 KB the
inputs are multiples of 1 / 1024 stored as int16 counts (exact), and ``mean_distances`` is stored as its strict upper triangle —
the four bytes of each little-endian fp32 in four rows, which deflate packs better — plus the few entries below the diagonal
that differ from their mirror image in the last bit; the diagonal is zero (checked).  tests/skeleton_init_ref.py reads them back.

Sampling fixtures (fps_*.npz): inputs, start and the indices of the reference's ``farthest_point_sample``
(utils/time_utils.py:461-482).  Only data is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim as S  # noqa: E402

S.install()
with S.quiet():
    import utils.time_utils as TU  # noqa: E402
    import skeleton_utils.extract_skeleton_utils as EX  # noqa: E402
    from skeleton_utils.mst_utils import gene_tree  # noqa: E402


GRID = 1024.0  # the inputs are multiples of 1 / 1024 and stored as int16 counts of it (exact)


def figure(per, F, seed, twigs=False):
    """(nodes (M, 3), all_deformed (F, M, 3)) fp32, multiples of 1 / GRID; nodes = the figure at rest."""
    rng = np.random.default_rng(seed)
    dirs = np.array([[0.0, 1.0, 0.1], [0.9, 0.35, -0.2], [-0.9, 0.4, 0.15], [0.45, -0.85, 0.25], [-0.5, -0.8, -0.3]])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    axes = np.cross(dirs, np.array([0.3, 0.2, 1.0]))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    s = np.arange(1, per + 1) / per
    limb = np.repeat(np.arange(5), per)
    arc = np.tile(s, 5)
    rest = dirs[limb] * arc[:, None] + 0.004 * rng.standard_normal((5 * per, 3))
    rest = np.concatenate([np.zeros((1, 3)), rest])
    limb = np.concatenate([[-1], limb])
    arc = np.concatenate([[0.0], arc])
    if twigs:  # one- to three-node side branches off every limb, moving with the part of the limb they sit on
        t_pos, t_limb, t_arc = [], [], []
        for l in range(5):
            for k, a in enumerate((0.3, 0.75, 0.9)):
                for step in range(1, k + 2):
                    t_pos.append(dirs[l] * a + axes[l] * step / per + 0.004 * rng.standard_normal(3))
                    t_limb.append(l)
                    t_arc.append(a)
        rest, limb, arc = np.concatenate([rest, np.array(t_pos)]), np.concatenate([limb, t_limb]), np.concatenate([arc, t_arc])

    def rot(axis, ang, p, centre):  # Rodrigues about `axis` through `centre`
        v = p - centre
        return centre + v * np.cos(ang) + np.cross(axis, v) * np.sin(ang) + axis * (v @ axis)[:, None] * (1 - np.cos(ang))

    frames = []
    for f in range(F):
        cur = rest.copy()
        for l in range(5):
            sel = limb == l
            outer = sel & (arc > 0.5)
            elbow = 0.9 * np.sin(2 * np.pi * f / F + 1.3 * l + 0.4)
            cur[outer] = rot(axes[l], elbow, cur[outer], 0.5 * dirs[l])
            swing = 0.6 * np.sin(2 * np.pi * f / F + 0.9 * l)
            cur[sel] = rot(axes[l], swing, cur[sel], np.zeros(3))
        frames.append(cur)
    q = lambda a: torch.from_numpy(((np.round(np.asarray(a) * GRID) + 0.0) / GRID).astype(np.float32))  # (+ 0.0: no negative zero, which int16 would not keep)  # noqa: E731
    return q(rest), q(np.stack(frames))


def stages(nodes, alld, sample):
    """The reference's stage functions one by one, as obtain_skeleton_tree chains them (:443-470)."""
    indices = torch.arange(0, nodes.shape[0]).int()
    select_nodes = nodes[sample]
    sel = alld[:, sample].unsqueeze(-2)
    mean_distances = torch.mean(torch.norm(sel - sel.transpose(1, 2), dim=-1), dim=0)
    prim = gene_tree(select_nodes.cpu().numpy(), mean_distances.cpu().numpy())
    select_indices = indices[sample]
    n1, p1, i1 = EX.adjust_arrow_dir(select_nodes, prim, select_indices)
    pruned, _ = EX.prune_tree(n1, alld[:, i1], p1, thres=1000)
    simplified = EX.simplify_tree(alld[:, i1], pruned, None)
    n1s = torch.stack(n1, dim=0)
    n2, p2, i2 = EX.adjust_arrow_dir(n1s, simplified, i1)
    return dict(mean_distances=mean_distances.numpy(), prim=np.array(prim, dtype=np.int64), parents1=np.array(p1, dtype=np.int64),
                indices1=torch.stack(i1).numpy(), pruned=np.asarray(pruned, dtype=np.int64), nodes1=n1s.numpy(),
                simplified=simplified.numpy().astype(np.int64), joints=torch.stack(n2).numpy(),
                parents=np.array(p2, dtype=np.int64), indices=torch.tensor(i2).numpy())


def whole(nodes, alld, seed):
    torch.manual_seed(seed)
    with S.quiet():
        j, p, i = EX.obtain_skeleton_tree(nodes.clone(), alld.clone(), None)
    return j, p, i


def skeleton_fixture(per, F, seed, twigs=False):
    name = "skelinit_per%d" % per + ("_twigs" if twigs else "")
    nodes, alld = figure(per, F, seed, twigs)
    M = nodes.shape[0]
    torch.manual_seed(seed)
    if M > 200:
        sample = TU.farthest_point_sample(nodes.unsqueeze(0), 200).squeeze()
        start = int(sample[0])
    else:
        sample, start = torch.arange(0, M).int(), -1
    with S.quiet():
        st = stages(nodes, alld, sample.long())
    j, p, i = whole(nodes, alld, seed)
    assert np.array_equal(j.numpy(), st["joints"]) and np.array_equal(p.numpy(), st["parents"]) and np.array_equal(i.numpy(), st["indices"])
    assert p.dtype == torch.int64 and i.dtype == torch.int32 and j.dtype == torch.float32
    for scale in (1 + 1e-5, 1 - 1e-5):  # the tree must not hang on the last bits of a distance
        js, ps, is_ = whole(nodes * scale, alld * scale, seed)
        if not (np.array_equal(ps.numpy(), p.numpy()) and np.array_equal(is_.numpy(), i.numpy())):
            raise SystemExit("%s: the reference's tree changes under a scaling of %r — not a usable fixture" % (name, scale))
    md = st.pop("mean_distances")
    assert not md.diagonal().any()
    iu = np.triu_indices(md.shape[0], 1)
    low = np.argwhere(np.tril(md != md.T, -1))  # (the strided mean over the frames leaves a few last-bit asymmetries)
    # select_key_frame (train_rig.py:164-174) with a coverage per frame, restated from its four lines
    cov = torch.from_numpy(np.random.default_rng(seed).integers(1000, 2000, F))
    dist = (alld - alld.mean(dim=0)[None]).norm(dim=-1).mean(dim=-1)
    _, near = torch.topk(dist, k=5, largest=False)
    key = int(near[torch.argmax(cov[near])])
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, nodes_q=np.round(nodes.numpy() * GRID).astype(np.int16), all_deformed_q=np.round(alld.numpy() * GRID).astype(np.int16),
                        grid=GRID, start=start,
                        sample=sample.numpy().astype(np.int64), mean_distances_triu_bytes=np.ascontiguousarray(md[iu].astype("<f4").view(np.uint8).reshape(-1, 4).T), mean_distances_low_at=low.astype(np.int32),
                        mean_distances_low=md[low[:, 0], low[:, 1]], coverage=cov.numpy(), key_frame=key,
                        key_frame_nearest=near.numpy(), **st)
    print("wrote", name, "nodes", M, "frames", F, "joints", len(p), "bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 100 * 1024


def fps_fixture(name, pts, npoint, seed):
    pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32))
    torch.manual_seed(seed)
    idx = TU.farthest_point_sample(pts.unsqueeze(0), npoint)[0]
    return name, pts, idx


def sampling_fixtures():
    rng = np.random.default_rng(77)
    # 70 001 points on a lattice of 1/64 (stored as int8: exact, and a quarter of the bytes): many workgroups, a ragged tail,
    # and equal distances everywhere
    lat = rng.integers(-128, 128, (70001, 3)).astype(np.int8)
    name, pts, idx = fps_fixture("fps_n70001_p64", lat.astype(np.float32) / 64.0, 64, 1)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), lattice_int8=lat, lattice_scale=1.0 / 64.0, start=int(idx[0]), indices=idx.numpy())
    print("wrote", name, os.path.getsize(os.path.join(HERE, name + ".npz")))
    cases = [("fps_n200_p200", rng.standard_normal((200, 3)), 200, 2),
             ("fps_n2050x2_p40", np.tile(rng.standard_normal((2050, 3)), (2, 1)), 40, 3),
             ("fps_same300_p5", np.tile(rng.standard_normal((1, 3)), (300, 1)), 5, 4),
             ("fps_n1_p1", rng.standard_normal((1, 3)), 1, 5)]
    for name, pts, npoint, seed in cases:
        name, pts, idx = fps_fixture(name, pts, npoint, seed)
        if name == "fps_n200_p200":
            assert sorted(idx.tolist()) == list(range(200))
        if name == "fps_n2050x2_p40":
            assert int(idx[1:].max()) < 2050
            pts = pts[:2050]  # (the test repeats them)
        if name == "fps_same300_p5":
            assert idx[1:].tolist() == [0, 0, 0, 0]
            pts = pts[:1]
        np.savez_compressed(os.path.join(HERE, name + ".npz"), points=pts.numpy(), start=int(idx[0]), indices=idx.numpy())
        print("wrote", name, os.path.getsize(os.path.join(HERE, name + ".npz")))


if __name__ == "__main__":
    for per, F, seed in ((12, 8, 11), (30, 16, 12), (60, 16, 13), (100, 12, 14)):
        skeleton_fixture(per, F, seed)
    skeleton_fixture(30, 16, 15, twigs=True)  # (short side branches: the first pass of prune_tree has work)
    sampling_fixtures()
