"""Golden vectors of the skeleton extraction WITH semantic labels (the symmetry pass, ``apply_symmetry``,
skeleton_utils/extract_skeleton_utils.py:177-255) from the REAL RigGS reference (CPU) — run in the build container only:
    python tests/golden/make_skeleton_symmetry_golden.py

Figures: those of make_skeleton_init_golden.py (``figure``: a centre and five limbs of ``per`` nodes) — (40, 24, 11, twigs) and
(60, 16, 7), where an all-zero label vector changes the reference's tree, (12, 24, 3), where it does not — and ``uneven_figure``,
the same construction with limbs of 20, 26, 23, 30 and 17 nodes that bend at different fractions of their length (``ELBOW``), so
that paired chains differ in length and in their cut, and the carried-over cut is re-mapped by arc length (it changes the tree).
Each figure is recorded with three label vectors (M,) int32:
    zero     all zero: what the reference's trainer passes without semantic maps — every pair of chains matches
    limbs    the limb's number + 1 (0 at the centre), limbs 1 and 2 sharing a label, as do limbs 3 and 4
    unique   every node a label of its own: no pair of chains passes ``semantic_thres``
For every vector the fixture holds the reference's ``simplified`` parents and the final (joints, parents, indices), or the flag
``index_error`` where the reference raises IndexError in ``simplify_tree``; besides that the inputs (multiples of 1 / 1024 as
int16 counts), the sample and its start, the stages in front of ``simplify_tree`` (``indices1``, ``pruned``) and the tree without
labels (``none_*``).  A fixture is written only if, for None and for all three vectors, tree and indices stay the same with all
inputs scaled by 1 + 1e-5 and by 1 - 1e-5.  Only data is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_skeleton_init_golden as G  # noqa: E402  (installs the reference through _ref_shim; its figure() and stage chain)

S, EX, TU, GRID = G.S, G.EX, G.TU, G.GRID
LABELS = ("zero", "limbs", "unique")
ELBOW = (0.5, 0.35, 0.6, 0.45, 0.65)  # uneven_figure: where along its length every limb bends
SHARED = np.array([0, 1, 2, 2, 4, 4])  # centre, then limbs 0 .. 4: limbs 1 and 2 share a label, so do 3 and 4


def limbs_of_figure(per, twigs):
    """The limb of every node of G.figure(per, ..., twigs): -1 at the centre (the layout of its ``limb`` array)."""
    limb = np.concatenate([[-1], np.repeat(np.arange(5), per)])
    if twigs:
        limb = np.concatenate([limb, np.repeat(np.arange(5), 1 + 2 + 3)])
    return limb


def uneven_figure(pers, F, seed):
    """G.figure with limbs of ``pers[l]`` nodes each (the same spacing along every limb: the limbs differ in length)."""
    rng = np.random.default_rng(seed)
    dirs = np.array([[0.0, 1.0, 0.1], [0.9, 0.35, -0.2], [-0.9, 0.4, 0.15], [0.45, -0.85, 0.25], [-0.5, -0.8, -0.3]])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    axes = np.cross(dirs, np.array([0.3, 0.2, 1.0]))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    step = 1.0 / max(pers)
    limb = np.concatenate([[-1]] + [np.full(p, l) for l, p in enumerate(pers)])
    arc = np.concatenate([[0.0]] + [np.arange(1, p + 1) * step for p in pers])
    rest = np.where(limb[:, None] >= 0, dirs[limb] * arc[:, None], 0.0)
    rest[1:] += 0.004 * rng.standard_normal((len(limb) - 1, 3))

    def rot(axis, ang, p, centre):
        v = p - centre
        return centre + v * np.cos(ang) + np.cross(axis, v) * np.sin(ang) + axis * (v @ axis)[:, None] * (1 - np.cos(ang))

    frames = []
    for f in range(F):
        cur = rest.copy()
        for l, p in enumerate(pers):
            sel = limb == l
            half = ELBOW[l] * p * step
            outer = sel & (arc > half)
            cur[outer] = rot(axes[l], 0.9 * np.sin(2 * np.pi * f / F + 1.3 * l + 0.4), cur[outer], half * dirs[l])
            cur[sel] = rot(axes[l], 0.6 * np.sin(2 * np.pi * f / F + 0.9 * l), cur[sel], np.zeros(3))
        frames.append(cur)
    q = lambda a: torch.from_numpy(((np.round(np.asarray(a) * GRID) + 0.0) / GRID).astype(np.float32))  # noqa: E731
    return q(rest), q(np.stack(frames)), limb


def label_vectors(limb):
    M = len(limb)
    return {"zero": np.zeros(M, np.int32), "limbs": SHARED[limb + 1].astype(np.int32), "unique": np.arange(1, M + 1, dtype=np.int32)}


def whole(nodes, alld, seed, labels):
    """The reference's obtain_skeleton_tree -> (joints, parents, indices) as numpy, or None where it raises IndexError."""
    torch.manual_seed(seed)
    try:
        with S.quiet():
            j, p, i = EX.obtain_skeleton_tree(nodes.clone(), alld.clone(), None if labels is None else torch.from_numpy(labels))
    except IndexError:
        return None
    return j.numpy(), p.numpy().astype(np.int64), i.numpy().astype(np.int32)


def same_tree(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def fixture(name, nodes, alld, limb, seed):
    M = nodes.shape[0]
    torch.manual_seed(seed)
    if M > 200:
        sample = TU.farthest_point_sample(nodes.unsqueeze(0), 200).squeeze()
        start = int(sample[0])
    else:
        sample, start = torch.arange(0, M).int(), -1
    with S.quiet():
        st = G.stages(nodes, alld, sample.long())  # (without labels)
    out = dict(nodes_q=np.round(nodes.numpy() * GRID).astype(np.int16), all_deformed_q=np.round(alld.numpy() * GRID).astype(np.int16),
               grid=GRID, start=start, seed=seed, sample=sample.numpy().astype(np.int64), indices1=st["indices1"], pruned=st["pruned"],
               none_simplified=st["simplified"], none_parents=st["parents"], none_indices=st["indices"])
    none = whole(nodes, alld, seed, None)
    assert np.array_equal(none[1], st["parents"]) and np.array_equal(none[2], st["indices"])
    differs = []
    for kind, labels in label_vectors(limb).items():
        ref = whole(nodes, alld, seed, labels)
        for scale in (1 + 1e-5, 1 - 1e-5):  # the tree must not hang on the last bits of a distance
            if not (same_tree(whole(nodes * scale, alld * scale, seed, labels), ref) and same_tree(whole(nodes * scale, alld * scale, seed, None), none)):
                raise SystemExit("%s / %s: the reference's tree changes under a scaling of %r — not a usable fixture" % (name, kind, scale))
        out["labels_" + kind] = labels
        out["index_error_" + kind] = ref is None
        if ref is None:
            differs.append(True)
            continue
        i1 = torch.from_numpy(st["indices1"]).long()
        try:
            with S.quiet():
                simplified = EX.simplify_tree(alld[:, i1], st["pruned"], torch.from_numpy(labels)[i1])
        except IndexError:
            raise SystemExit("%s / %s: simplify_tree raises on its own but not inside obtain_skeleton_tree" % (name, kind))
        out["simplified_" + kind] = simplified.numpy().astype(np.int64)
        out["joints_" + kind], out["parents_" + kind], out["indices_" + kind] = ref
        differs.append(not same_tree(ref, none))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", name, "nodes", M, "frames", alld.shape[0], "joints without labels", len(none[1]),
          {k: ("IndexError" if out["index_error_" + k] else len(out["parents_" + k])) for k in LABELS}, "differs from None", differs,
          "bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 100 * 1024
    return differs


if __name__ == "__main__":
    differing = 0
    for name, (per, F, seed, twigs) in (("skelsym_per40_twigs", (40, 24, 11, True)), ("skelsym_per60", (60, 16, 7, False)),
                                         ("skelsym_per12", (12, 24, 3, False))):
        nodes, alld = G.figure(per, F, seed, twigs)
        differing += sum(fixture(name, nodes, alld, limbs_of_figure(per, twigs), seed))
    nodes, alld, limb = uneven_figure((20, 26, 23, 30, 17), 16, 21)
    differing += sum(fixture("skelsym_uneven", nodes, alld, limb, 21))
    assert differing >= 2, "the symmetry pass changes the tree in fewer than two fixtures"
