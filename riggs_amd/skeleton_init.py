"""From a trained stage 1 to the start of stage 2: the skeleton — joints, a parent list, the stage-1 node every joint came from —
extracted once from the control nodes' trajectories (``TrainRig.init_skeleton_info`` / ``precompute_deformations``,
train_rig.py:117-262, over ``obtain_skeleton_tree``, skeleton_utils/extract_skeleton_utils.py:426-471).

The device work is the farthest-point sample of the nodes (csrc/fps.hip through riggs_amd/fps.py), the (S, S) mean over the frames
of the pairwise node distances (torch ops, S <= 200) and F forward passes of the stage-1 warp.  Everything after that is a graph
of at most 200 vertices: host code over numpy, written from the algorithm each stage of the reference runs and keeping its
behaviour where that behaviour looks accidental (each such point is named where it happens) — a skeleton extracted here is the
skeleton the reference extracts from the same trajectories.

The symmetry pass (``apply_symmetry``, extract_skeleton_utils.py:177-255) needs per-camera semantic maps that one dataset has:
``seg_labels`` other than None raises NotImplementedError.
"""
from __future__ import annotations

import os
from collections import deque

import numpy as np
import torch

SAMPLE_NODES = 200  # extract_skeleton_utils.py:438-439


# ---- the spanning tree (skeleton_utils/mst_utils.py:352-361 gene_tree -> Prim's algorithm from vertex 2) ------------------
def prim_tree(weights, start=2):
    """Prim's minimum spanning tree of a dense symmetric weight matrix, grown from ``start``: (S,) parents, -1 at ``start``.
    As the reference runs it: the next vertex is the cheapest one outside the tree with the LOWEST index on ties, a vertex's
    key is lowered only by a strictly smaller edge, and an edge of weight <= 0 does not exist (two nodes with identical
    trajectories are not connected directly)."""
    w = np.asarray(weights)
    S = w.shape[0]
    if S <= start:
        raise ValueError("the skeleton tree grows from vertex %d: at least %d nodes are needed" % (start, start + 1))
    key = np.full(S, np.inf)
    parent = np.full(S, -1, dtype=np.int64)
    inside = np.zeros(S, dtype=bool)
    key[start] = 0.0
    for _ in range(S):
        cand = np.where(inside, np.inf, key)
        u = int(np.argmin(cand))  # (the first minimum: the lowest index)
        if not np.isfinite(cand[u]):
            raise ValueError("the node graph is not connected by edges of positive weight")
        inside[u] = True
        row = w[u]
        lower = (row > 0) & ~inside & (key > row)
        key[lower] = row[lower]
        parent[lower] = u
    return parent


# ---- re-rooting (extract_skeleton_utils.py:59-85 adjust_arrow_dir, :7-57 its two searches) ------------------------------
def _neighbours(parents):
    n = len(parents)
    nb = [[] for _ in range(n)]
    for i in range(n):
        p = int(parents[i])
        if p >= 0:  # (-1: the root, -2: a vertex an earlier stage removed)
            nb[i].append(p)
            nb[p].append(i)
    return nb


def _reach_of_end(src, nb, is_end):
    """What the reference scores a root candidate with (:7-29): the number of vertices ENQUEUED by a breadth-first search from
    ``src`` up to the moment it dequeues an end point — not the depth of that end point; -1 when it meets none."""
    seen = np.zeros(len(nb), dtype=bool)
    seen[src] = True
    queue = deque([src])
    count = 0
    while queue:
        v = queue.popleft()
        if is_end[v]:
            return count
        for u in nb[v]:
            if not seen[u]:
                seen[u] = True
                queue.append(u)
                count += 1
    return -1


def reroot(parents):
    """The tree re-rooted at the junction (degree >= 3) with the largest score above (the first on ties) and renumbered in
    breadth-first order: ``(order, new_parents)`` — ``order[k]`` the old vertex that becomes vertex k, ``new_parents`` with
    -1 at 0.  Vertices without an edge (removed ones) drop out."""
    nb = _neighbours(parents)
    degree = np.array([len(x) for x in nb])
    is_end = degree == 1
    cands = [i for i in range(len(nb)) if degree[i] >= 3]
    if not cands:
        raise ValueError("the node tree has no junction (a vertex of degree >= 3) to root the skeleton at")
    root = cands[int(np.argmax(np.array([_reach_of_end(i, nb, is_end) for i in cands])))]
    seen = np.zeros(len(nb), dtype=bool)
    seen[root] = True
    queue = deque([root])
    order, new_parents = [], [-1]
    while queue:
        v = queue.popleft()
        order.append(v)
        for u in nb[v]:
            if not seen[u]:
                seen[u] = True
                queue.append(u)
                new_parents.append(len(order) - 1)
    return np.array(order, dtype=np.int64), np.array(new_parents, dtype=np.int64)


# ---- pruning (extract_skeleton_utils.py:319-423 prune_tree) --------------------------------------------------------------
def prune_tree(nodes, parents):
    """Two passes over the re-rooted tree: ``(new_parents, nodes)`` with -2 at every removed vertex and the merged junctions'
    positions written into (a copy of) ``nodes``.

    1. A leaf whose walk towards the root meets a vertex with more than one child within four steps is removed together with
       the vertices it passed (short side twigs).  The walk runs while ``parent >= -1``: at the root it steps to "vertex -1",
       which Python reads as the LAST vertex — its child list, its parent.  That is kept.
    2. From the highest index down, a junction whose walk up meets another junction within three single-child vertices is
       merged into it: the upper junction moves to the mean of the two and of the vertices between them, takes the lower
       one's children, and the lower junction and the vertices between are removed.  ``visited[parent]`` is read with the
       parent's -1 / -2 as it stands (the last / second-to-last vertex), as the reference does.
    The reference also accumulates an edge length along walk 1 and never reads it (its ``thres`` is unused): left out."""
    n = len(parents)
    parents = [int(p) for p in parents]
    nodes = np.array(nodes, dtype=np.float32, copy=True)
    new_parents = list(parents)
    children = [[] for _ in range(n)]
    for i, p in enumerate(parents):
        if p >= 0:
            children[p].append(i)

    def unlink(child, parent):
        if child in children[parent]:
            children[parent].remove(child)

    for leaf in range(n):  # :333-360
        if children[leaf]:
            continue
        p, passed, prune = parents[leaf], [], False
        while p >= -1 and len(passed) < 4:
            if len(children[p]) > 1:
                prune = True
                break
            passed.append(p)
            p = parents[p]
        if prune:
            new_parents[leaf] = -2
            unlink(leaf, parents[leaf])
            for v in passed:
                new_parents[v] = -2
                unlink(v, parents[v])

    visited = np.zeros(n, dtype=bool)
    for c in range(n - 1, -1, -1):  # :363-421
        p = new_parents[c]
        if visited[c] or visited[p] or p < 0 or len(children[c]) <= 1:
            continue
        passed, upper = [], -2
        while len(passed) < 3 and p >= 0:
            if len(children[p]) == 1:
                passed.append(p)
                p = new_parents[p]
            else:
                if len(children[p]) > 1:
                    upper = p
                break
        if upper < 0:
            continue
        pos = nodes[c] + nodes[upper]
        for v in passed:
            pos = pos + nodes[v]
        nodes[upper] = pos / (2 + len(passed))  # (fp32, summed in this order: the joint positions are the reference's bits)
        visited[upper] = visited[c] = True
        for g in children[c]:
            if g not in children[upper]:
                children[upper].append(g)
                new_parents[g] = upper
        new_parents[c] = -2
        children[c] = []
        for v in passed:
            unlink(v, new_parents[v])
            visited[v] = True
            new_parents[v] = -2
            children[v] = []
    return np.array(new_parents, dtype=np.int64), nodes


# ---- path simplification (extract_skeleton_utils.py:257-301 simplify_tree, :122-161 compute_insert_points) --------------
def _segment_distance(a, b, p):
    """Mean over the frames of the distance from ``p`` (F, n, 3) to the segment a-b (F, 1, 3) (:99-120, with its two 1e-6)."""
    ab = b - a
    t = ((p - a) * ab).sum(-1, keepdims=True) / np.maximum((ab * ab).sum(-1, keepdims=True), 1e-6)
    s = a + np.clip(t, 0.0, 1.0) * ab
    return np.sqrt(((s - p) ** 2).sum(-1) + 1e-6).mean(0)


def _split_path(path, pts, dist_thres, num_thres=3):
    """A chain of vertices replaced by as few straight pieces as keep every vertex within ``dist_thres`` of its piece (mean over
    the frames): breadth-first bisection at the vertex that is farthest from the chord.  Pieces as pairs of positions in
    ``path``.  A piece that still needs a split once more than ``num_thres`` pieces are settled is dropped, vertices and all
    (:155-156).  (The reference subtracts 0.1 of a "distance to the nearer end" from the score it maximises, :143-149, but takes
    that distance with ``.norm(-1)`` — the p = -1 norm over ALL elements, one number for the whole chain — so the subtraction
    shifts every score alike and the choice is the plain maximum; that is what is kept.)"""
    pieces = []
    queue = deque([(0, len(path) - 1)])
    while queue:
        a, b = queue.popleft()
        if b - a < 2:
            pieces.append((a, b))
            continue
        pa, pb, pm = pts[:, path[a:a + 1]], pts[:, path[b:b + 1]], pts[:, path[a + 1:b]]
        d_ab = _segment_distance(pa, pb, pm)
        if d_ab.max() < dist_thres:
            pieces.append((a, b))
            continue
        if len(pieces) > num_thres:
            continue
        m = int(np.argmax(d_ab)) + a + 1
        queue.append((a, m))
        queue.append((m, b))
    return pieces


def simplify_tree(all_points, parents, dist_thres=1.0):
    """Every chain between two key vertices (leaf or junction below, junction or root above) is cut into straight pieces; the
    ends of the pieces stay, with the upper end of its piece as parent, everything else becomes -2.  The threshold is
    ``dist_thres`` mean edge lengths of the tree (:307-316).  Vertex 0 is made the root whatever the pieces say (:300).
    A chain that runs past the root ends in "vertex -1", read as the last vertex like everywhere in Python.
    ``all_points`` (F, n, 3): the vertices' trajectories; distances are taken in float64."""
    pts = np.asarray(all_points, dtype=np.float64)
    parents = np.asarray(parents, dtype=np.int64)
    n = len(parents)
    children = [[] for _ in range(n)]
    for i in range(n):
        if parents[i] >= 0:
            children[parents[i]].append(i)
    is_key = np.array([len(c) > 1 for c in children])
    has = parents >= 0
    mean_edge = np.linalg.norm(pts[:, parents[has]] - pts[:, has], axis=-1).mean(0).mean()
    new_parents = np.full(n, -2, dtype=np.int64)
    for v in range(n):
        p = int(parents[v])
        if p < 0 or not (len(children[v]) == 0 or is_key[v]):
            continue
        path = [v]
        while True:
            path.append(p)
            if p < 0 or is_key[p]:
                break
            p = int(parents[p])
        for a, b in _split_path(path, pts, dist_thres * mean_edge):
            new_parents[path[a]] = path[b]
    new_parents[0] = -1
    return new_parents


# ---- the whole extraction ----------------------------------------------------------------------------------------------
def mean_pairwise_distances(points):
    """(F, S, 3) -> (S, S): the mean over the frames of the pairwise distances (:445-448), torch ops on the points' device."""
    return torch.norm(points.unsqueeze(-2) - points.unsqueeze(-2).transpose(1, 2), dim=-1).mean(dim=0)


def tree_from_samples(select_nodes, sample_indices, mean_distances, all_deformed_nodes):
    """The host stages of ``obtain_skeleton_tree`` (:450-471) on numpy arrays — the sampled nodes (S, 3), their indices (S,), the
    (S, S) mean distances and all nodes' trajectories (F, M, 3): a dict of every stage's result (``prim``, ``order1`` /
    ``parents1`` / ``indices1`` of the first re-rooting, ``pruned``, ``simplified``) and the final ``joints`` (fp32),
    ``parents`` (int64), ``indices`` (int32)."""
    select_nodes = np.asarray(select_nodes, dtype=np.float32)
    sample_indices = np.asarray(sample_indices)
    traj = np.asarray(all_deformed_nodes)
    prim = prim_tree(np.asarray(mean_distances), 2)
    order1, parents1 = reroot(prim)
    nodes1, indices1 = select_nodes[order1], sample_indices[order1]
    pruned, nodes1 = prune_tree(nodes1, parents1)
    simplified = simplify_tree(traj[:, indices1], pruned)
    order2, parents2 = reroot(simplified)
    return {"prim": prim, "order1": order1, "parents1": parents1, "indices1": indices1.astype(np.int32), "pruned": pruned,
            "simplified": simplified, "joints": nodes1[order2], "parents": parents2, "indices": indices1[order2].astype(np.int32)}


def obtain_skeleton_tree(nodes, all_deformed_nodes, seg_labels=None, start=None):
    """The sparse skeleton of the control nodes (extract_skeleton_utils.py:426-471).  ``nodes`` (M, 3): the nodes at the template
    frame; ``all_deformed_nodes`` (F, M, 3): at every training frame.  Returns ``(joints (J, 3) fp32, parents (J,) int64 with
    -1 at joint 0, indices (J,) int32)`` on the nodes' device; ``indices[j]`` is the node joint j came from.  More than 200 nodes
    are sampled down to 200 by farthest points from a random start (``start``: that index, for a reproducible run)."""
    if seg_labels is not None:
        raise NotImplementedError("seg_labels: the symmetry pass over semantic labels (apply_symmetry) is not part of this "
                                  "library — it needs per-camera semantic maps; pass seg_labels=None")
    from .gaussian_model import farthest_point_sample
    dev = nodes.device
    nodes, all_deformed_nodes = nodes.detach(), all_deformed_nodes.detach()
    M = nodes.shape[0]
    if M > SAMPLE_NODES:
        st = None if start is None else torch.as_tensor(start, dtype=torch.long).reshape(1)
        sample = farthest_point_sample(nodes.float().unsqueeze(0), SAMPLE_NODES, start=st)[0]
    else:
        sample = torch.arange(M, device=dev)
    mean_distances = mean_pairwise_distances(all_deformed_nodes[:, sample])
    out = tree_from_samples(nodes[sample].float().cpu().numpy(), sample.cpu().numpy(), mean_distances.cpu().numpy(),
                            all_deformed_nodes.float().cpu().numpy())
    return (torch.from_numpy(out["joints"]).to(dev), torch.from_numpy(out["parents"]).to(dev),
            torch.from_numpy(out["indices"]).to(dev))


def select_key_frame(d_nodes, coverage=None, manually_key_frame=-1):
    """The template frame (train_rig.py:164-174): among the five frames whose nodes lie closest to the nodes' mean over the
    frames, the one with the largest ``coverage`` (F,) — a per-frame mask area, what ``cal_max_coverage_view`` (:149-160) sums
    from the cameras' alpha masks; the first on ties, so without ``coverage`` the closest frame.  ``manually_key_frame >= 0``
    wins."""
    if manually_key_frame >= 0:
        return int(manually_key_frame)
    d_nodes = d_nodes.detach()
    dist = (d_nodes - d_nodes.mean(dim=0)[None]).norm(dim=-1).mean(dim=-1)
    _, nearest = torch.topk(dist, k=min(5, dist.shape[0]), largest=False)
    if coverage is None:
        return int(nearest[0])
    area = torch.as_tensor(coverage).to(nearest.device)[nearest]
    return int(nearest[torch.argmax(area)])


# ---- skeleton_tree.npz (train_rig.py:233, :243-254) -----------------------------------------------------------------------
def save_skeleton_tree(path, joints, parent_indices, joint_node_indices, template_idx):
    """The reference's file: ``nodes`` fp32 (J, 3), ``parents`` int64 (J,), ``indices`` int32 (J,), ``template_idx`` int64 ()."""
    np.savez(path, nodes=torch.as_tensor(joints).detach().cpu().numpy().astype(np.float32),
             parents=torch.as_tensor(parent_indices).cpu().numpy().astype(np.int64),
             indices=torch.as_tensor(joint_node_indices).cpu().numpy().astype(np.int32), template_idx=int(template_idx))


def load_skeleton_tree(path, device="cpu"):
    """``skeleton_tree_info`` from the file (the ``init=False`` branch, :243-254): joints fp32, the two index lists int64."""
    if not os.path.exists(path):
        raise FileNotFoundError("no saved skeleton tree at %s" % path)
    z = np.load(path)
    return {"joints": torch.from_numpy(z["nodes"]).float().to(device), "parent_indices": torch.from_numpy(z["parents"]).long().to(device),
            "joint_node_indices": torch.from_numpy(z["indices"]).long().to(device), "template_idx": int(z["template_idx"])}


# ---- train_rig.py:192-262 and the tail of init_skeleton_info (:135-141) --------------------------------------------------
@torch.no_grad()
def precompute_deformations(deform, gaussians, fids, coverage=None, model_path=None, num_gs_sample=0, manually_key_frame=-1):
    """The trained stage 1 at every training frame, and the skeleton drawn from it.  ``deform``: a ``ControlNodeWarp`` (or a
    model holding one as ``.deform``); ``gaussians``: the stage-1 ``GaussianModel``; ``fids`` (F,): the training frames' times,
    visited in ascending order (``coverage`` (F,), the frames' mask areas, is given in the order of ``fids``).

    Returns ``(pretrain_deform_info, skeleton_tree_info, template_offsets)``: the stacked ``d_xyz`` (F, N, 3), ``d_nodes``
    (F, M, 3), ``d_rotation``, ``d_scaling`` and ``d_joints`` = ``d_nodes[:, joint_node_indices]``; ``joints``,
    ``parent_indices``, ``joint_node_indices``, ``template_idx`` (an index into the sorted frames).  As in the reference the
    template frame becomes the rest pose: its ``d_xyz`` — the template offsets — is ADDED to ``gaussians._xyz`` and subtracted
    from every frame's ``d_xyz``.  ``num_gs_sample > 10`` first thins the Gaussians (``sampling_and_prune``); ``model_path``:
    where ``skeleton_tree.npz`` and ``skeleton.obj`` are written."""
    from .skeleton import write_to_obj
    warp = getattr(deform, "deform", deform)
    if num_gs_sample > 10:
        gaussians.sampling_and_prune(num_gs_sample)
    dev = warp.nodes.device
    fids = torch.as_tensor(fids, dtype=torch.float32).reshape(-1)
    order = torch.argsort(fids, stable=True)
    fids = fids[order].to(dev)
    if coverage is not None:
        coverage = torch.as_tensor(coverage).reshape(-1).cpu()[order]
    xyz = gaussians.get_xyz.detach()
    stacks = {"d_xyz": [], "d_nodes": [], "d_rotation": [], "d_scaling": []}
    for i in range(fids.shape[0]):
        d = warp(xyz, warp.expand_time(fids[i:i + 1]), feature=gaussians.feature, motion_mask=gaussians.motion_mask)
        for k in stacks:
            stacks[k].append(d[k].detach())
    info = {k: torch.stack(v) for k, v in stacks.items()}
    template_idx = select_key_frame(info["d_nodes"], coverage, manually_key_frame)
    joints, parent_indices, joint_node_indices = obtain_skeleton_tree(info["d_nodes"][template_idx], info["d_nodes"], None)
    tree = {"joints": joints, "parent_indices": parent_indices, "joint_node_indices": joint_node_indices, "template_idx": int(template_idx)}
    if model_path is not None:
        os.makedirs(model_path, exist_ok=True)
        save_skeleton_tree(os.path.join(model_path, "skeleton_tree.npz"), joints, parent_indices, joint_node_indices, template_idx)
        write_to_obj(joints.cpu(), os.path.join(model_path, "skeleton.obj"), parent_indices.cpu())
    info["d_joints"] = info["d_nodes"][:, joint_node_indices.long()]
    template_offsets = info["d_xyz"][template_idx].clone()
    gaussians._xyz.data = xyz + template_offsets
    info["d_xyz"] = info["d_xyz"] - template_offsets[None]
    return info, tree, template_offsets


def skeleton_model_from_tree(skeleton_tree_info, stage1=None, **kwargs):
    """The stage-2 model on an extracted (or loaded) tree (train_rig.py:81-88): ``SkeletonModel(joints=, parent_indices=,
    **kwargs)``, and with the stage-1 warp (``stage1``: a ``ControlNodeWarp`` or a model holding one as ``.deform``) every
    joint starts with the radius of the node it came from."""
    from .skeleton import SkeletonModel
    model = SkeletonModel(joints=skeleton_tree_info["joints"], parent_indices=skeleton_tree_info["parent_indices"], **kwargs)
    if stage1 is not None:
        warp = getattr(stage1, "deform", stage1)
        idx = skeleton_tree_info["joint_node_indices"].long().to(warp._node_radius.device)
        model.deform._node_radius.data = warp._node_radius.detach()[idx].clone().to(model.deform._node_radius.device)
    return model
