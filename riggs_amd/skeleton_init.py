"""From a trained stage 1 to the start of stage 2: the skeleton — joints, a parent list, the stage-1 node every joint came from —
extracted once from the control nodes' trajectories (``TrainRig.init_skeleton_info`` / ``precompute_deformations``,
train_rig.py:117-262, over ``obtain_skeleton_tree``, skeleton_utils/extract_skeleton_utils.py:426-471).

The device work is the farthest-point sample of the nodes (csrc/fps.hip through riggs_amd/fps.py), the (S, S) mean over the frames
of the pairwise node distances (torch ops, S <= 200) and F forward passes of the stage-1 warp.  Everything after that is a graph
of at most 200 vertices: host code over numpy, written from the algorithm each stage of the reference runs and keeping its
behaviour where that behaviour looks accidental (each such point is named where it happens) — a skeleton extracted here is the
skeleton the reference extracts from the same trajectories.

The symmetry pass (``apply_symmetry``, extract_skeleton_utils.py:177-255) runs when ``obtain_skeleton_tree`` is given a label per
node together with ``symmetry=True`` (opt-in: nothing a caller does today changes its tree).  The reference's trainer always
gives one: the median over the training frames of the label each node projects onto in the frame's semantic map, and zero for a camera without a map (train_rig.py:129-131, 177-190, 227) — so all zeros for a dataset without
maps, which is not the same as no labels.  ``node_semantic_labels`` computes labels and median for all frames in one launch
(csrc/semantic.hip); ``precompute_deformations(..., cameras=, symmetry=True)`` is the trainer's call.
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


# ---- the symmetry pass (extract_skeleton_utils.py:165-255 compute_single_source_path_distance, apply_symmetry) ------------
def compute_single_source_path_distance(all_points, path):
    """(len(path),) arc length along ``path`` from its first vertex, each edge the mean over the frames of its length (:165-173).
    A trailing -1 (a chain that ran past the root) reads the last vertex."""
    pts = np.asarray(all_points, dtype=np.float64)
    path = np.asarray(path, dtype=np.int64)
    edge = np.linalg.norm(pts[:, path[:-1]] - pts[:, path[1:]], axis=-1).mean(0)
    return np.concatenate([[0.0], np.cumsum(edge)])


def apply_symmetry(paths, edge_idxs, all_points, semantic_label, length_thres=0.7, semantic_thres=0.6):
    """Chains that look like each other's mirror image get the same cut (:177-255).  ``paths``: the chains of ``simplify_tree``,
    each with its trailing parent entry; ``edge_idxs``: per chain its pieces as pairs of positions in it; ``semantic_label`` (n,)
    integers per vertex.  Chains are paired greedily — chain i with the later chain j of the best score
    ``length_ratio + semantic_score`` among those with ``length_ratio = 1 - |len_i - len_j| / max(len_i, len_j) > length_thres``
    and ``semantic_score = |labels_i & labels_j| / max(|labels_i|, |labels_j|) > semantic_thres`` (label SETS) — and in each pair
    the pieces of the chain whose piece count is nearer 2 are carried over to the other chain by normalised arc length.
    Returns ``edge_idxs`` (the same list, the carried-over entries replaced); nothing changes when no pair qualifies.
    Kept from the reference although it looks accidental: see the comments."""
    label = np.asarray(semantic_label)
    # the labels of a chain INCLUDE its trailing parent entry; where that is -1 (past the root) it reads the LAST label
    sets = [np.unique(label[np.asarray(p, dtype=np.int64)]) for p in paths]
    pairs = []
    taken = np.zeros(len(paths), dtype=bool)
    for i in range(len(paths)):
        if taken[i]:  # (only as the first of a pair: a taken chain may still be chosen as j by a later i)
            continue
        best_score, best = 0, -1
        for j in range(i + 1, len(paths)):
            len_i, len_j = len(paths[i]), len(paths[j])
            if len(edge_idxs[i]) == 1 and len(edge_idxs[j]) == 1:  # skipped only when BOTH chains are one piece
                continue
            length_ratio = 1.0 - abs(len_i - len_j) / (max(len_i, len_j) + 1e-10)
            if length_ratio > length_thres:
                semantic_score = len(np.intersect1d(sets[i], sets[j])) / (max(len(sets[i]), len(sets[j])) + 1e-10)
                if semantic_score > semantic_thres:
                    score = length_ratio + semantic_score
                    if score > best_score:  # strictly: the first best wins
                        best_score, best = score, j
        if best >= 0:
            pairs.append((i, best))
            taken[best] = True
    for first, second in pairs:
        # the chain whose piece count is nearer 2 gives its cut to the other; on equality that is the SECOND of the pair
        if abs(len(edge_idxs[first]) - 2) < abs(len(edge_idxs[second]) - 2):
            select, other = first, second
        else:
            select, other = second, first
        pieces = sorted(edge_idxs[select], key=lambda e: e[0])
        d_select = compute_single_source_path_distance(all_points, paths[select])
        d_other = compute_single_source_path_distance(all_points, paths[other])
        d_select, d_other = d_select / d_select[-1], d_other / d_other[-1]  # normalised by the last entry (the whole chain)
        carried = []
        for k in range(len(pieces)):
            start = 0 if k == 0 else int(np.argmin(np.abs(d_select[pieces[k][0]] - d_other)))
            # the reference compares the PIECE counter with the chain's LENGTH (a chain of n entries has at most n - 1 pieces, so
            # this never holds) and would then take a vertex ID, paths[other][-1], where a position in the chain is meant;
            # simplify_tree raises IndexError where such an entry does not index the chain, as the reference does
            if k == len(paths[select]) - 1:
                end = int(paths[other][-1])
            else:
                end = int(np.argmin(np.abs(d_select[pieces[k][1]] - d_other)))
            carried.append((start, end))
        edge_idxs[other] = carried
    return edge_idxs


def simplify_tree(all_points, parents, semantic_label=None, dist_thres=1.0):
    """Every chain between two key vertices (leaf or junction below, junction or root above) is cut into straight pieces; the
    ends of the pieces stay, with the upper end of its piece as parent, everything else becomes -2.  The threshold is
    ``dist_thres`` mean edge lengths of the tree (:307-316).  Vertex 0 is made the root whatever the pieces say (:300).
    A chain that runs past the root ends in "vertex -1", read as the last vertex like everywhere in Python.
    ``all_points`` (F, n, 3): the vertices' trajectories; distances are taken in float64.  ``semantic_label`` (n,) integers, or
    None: with labels the pieces of all chains go through ``apply_symmetry`` before they are written (:294-295)."""
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
    paths, edge_idxs = [], []
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
        paths.append(path)
        edge_idxs.append(_split_path(path, pts, dist_thres * mean_edge))
    if semantic_label is not None:
        semantic_label = np.asarray(semantic_label).reshape(-1)
        if semantic_label.shape[0] != n:
            raise ValueError("simplify_tree: %d labels for %d vertices" % (semantic_label.shape[0], n))
        edge_idxs = apply_symmetry(paths, edge_idxs, pts, semantic_label)
    new_parents = np.full(n, -2, dtype=np.int64)
    for path, pieces in zip(paths, edge_idxs):
        for a, b in pieces:
            if not (-len(path) <= a < len(path) and -len(path) <= b < len(path)):
                raise IndexError("simplify_tree: the symmetry pass carried the piece (%d, %d) over to a chain of %d entries — "
                                 "apply_symmetry took a vertex id for a position in the chain, as the reference does" % (a, b, len(path)))
            new_parents[path[a]] = path[b]
    new_parents[0] = -1
    return new_parents


# ---- the whole extraction ----------------------------------------------------------------------------------------------
def mean_pairwise_distances(points):
    """(F, S, 3) -> (S, S): the mean over the frames of the pairwise distances (:445-448), torch ops on the points' device."""
    return torch.norm(points.unsqueeze(-2) - points.unsqueeze(-2).transpose(1, 2), dim=-1).mean(dim=0)


def tree_from_samples(select_nodes, sample_indices, mean_distances, all_deformed_nodes, seg_labels=None):
    """The host stages of ``obtain_skeleton_tree`` (:450-471) on numpy arrays — the sampled nodes (S, 3), their indices (S,), the
    (S, S) mean distances and all nodes' trajectories (F, M, 3): a dict of every stage's result (``prim``, ``order1`` /
    ``parents1`` / ``indices1`` of the first re-rooting, ``pruned``, ``simplified``) and the final ``joints`` (fp32),
    ``parents`` (int64), ``indices`` (int32).  ``seg_labels`` (M,) integers per node, or None: the symmetry pass of
    ``simplify_tree``, which reads them by the re-rooted tree's node indices (:459)."""
    select_nodes = np.asarray(select_nodes, dtype=np.float32)
    sample_indices = np.asarray(sample_indices)
    traj = np.asarray(all_deformed_nodes)
    prim = prim_tree(np.asarray(mean_distances), 2)
    order1, parents1 = reroot(prim)
    nodes1, indices1 = select_nodes[order1], sample_indices[order1]
    pruned, nodes1 = prune_tree(nodes1, parents1)
    simplified = simplify_tree(traj[:, indices1], pruned, None if seg_labels is None else np.asarray(seg_labels).reshape(-1)[indices1])
    order2, parents2 = reroot(simplified)
    return {"prim": prim, "order1": order1, "parents1": parents1, "indices1": indices1.astype(np.int32), "pruned": pruned,
            "simplified": simplified, "joints": nodes1[order2], "parents": parents2, "indices": indices1[order2].astype(np.int32)}


def obtain_skeleton_tree(nodes, all_deformed_nodes, seg_labels=None, start=None, symmetry=False):
    """The sparse skeleton of the control nodes (extract_skeleton_utils.py:426-471).  ``nodes`` (M, 3): the nodes at the template
    frame; ``all_deformed_nodes`` (F, M, 3): at every training frame.  Returns ``(joints (J, 3) fp32, parents (J,) int64 with
    -1 at joint 0, indices (J,) int32)`` on the nodes' device; ``indices[j]`` is the node joint j came from.  More than 200 nodes
    are sampled down to 200 by farthest points from a random start (``start``: that index, for a reproducible run).
    ``seg_labels`` with ``symmetry=True``: an (M,) integer tensor on any device — a semantic label per node
    (``node_semantic_labels``'s median, or zeros: what the reference's trainer passes); the chains of the tree then go through
    the symmetry pass (``apply_symmetry``).  An all-zero vector is NOT the same as None: every pair of chains then matches
    semantically.  The pass is opt-in: labels without ``symmetry=True`` raise NotImplementedError, as they always have — a caller
    written before the pass existed does not silently get another tree — and ``symmetry=True`` needs labels."""
    if seg_labels is not None and not symmetry:
        raise NotImplementedError("seg_labels: the symmetry pass over semantic labels (apply_symmetry) is opt-in — pass "
                                  "symmetry=True with the labels to run it, or seg_labels=None for the tree without it")
    if symmetry and seg_labels is None:
        raise ValueError("symmetry=True needs seg_labels: a label per node (zeros are what the reference passes without maps)")
    from .gaussian_model import farthest_point_sample
    dev = nodes.device
    nodes, all_deformed_nodes = nodes.detach(), all_deformed_nodes.detach()
    M = nodes.shape[0]
    if seg_labels is not None:
        seg_labels = torch.as_tensor(seg_labels).detach()
        if seg_labels.is_floating_point() or seg_labels.is_complex() or seg_labels.dtype is torch.bool or seg_labels.numel() != M:
            raise ValueError("seg_labels must be an integer tensor of one label per node (%d), got %s %s"
                             % (M, tuple(seg_labels.shape), seg_labels.dtype))
        seg_labels = seg_labels.reshape(-1).cpu().numpy()
    if M > SAMPLE_NODES:
        st = None if start is None else torch.as_tensor(start, dtype=torch.long).reshape(1)
        sample = farthest_point_sample(nodes.float().unsqueeze(0), SAMPLE_NODES, start=st)[0]
    else:
        sample = torch.arange(M, device=dev)
    mean_distances = mean_pairwise_distances(all_deformed_nodes[:, sample])
    out = tree_from_samples(nodes[sample].float().cpu().numpy(), sample.cpu().numpy(), mean_distances.cpu().numpy(),
                            all_deformed_nodes.float().cpu().numpy(), seg_labels)
    return (torch.from_numpy(out["joints"]).to(dev), torch.from_numpy(out["parents"]).to(dev),
            torch.from_numpy(out["indices"]).to(dev))


# ---- the nodes' semantic labels (train_rig.py:129-131, 177-190, 215-216, 227) on csrc/semantic.hip ------------------------
@torch.no_grad()
def node_semantic_labels(d_nodes, cameras):
    """A semantic label per control node from the training cameras' semantic maps, all frames in one launch
    (``riggs_node_semantic_labels``): node m at frame f is projected into camera f as ``project_nodes_to_2d_elements`` does, the
    pixel truncated and clamped into the image as ``set_semantic_label`` does, and the camera's map read there.

    ``d_nodes`` (F, M, 3) fp32 on the device; ``cameras``: F objects in the order of ``d_nodes``' first axis, with
    ``world_view_transform``, ``FoVx``, ``FoVy``, ``image_height``, ``image_width``, optionally ``K`` and optionally
    ``semantic_seg`` — an (H, W) integer tensor (moved to the device and cast to int32 as needed) or None: such a camera's row
    is all zero.  Returns ``(labels (F, M) fp32, median (M,) int32)`` on the device: the reference's ``nodes_semantic_label``
    and its ``torch.median(dim=0).values.int()`` (the lower median), what ``obtain_skeleton_tree`` takes as ``seg_labels``.
    1 <= F <= 1024, 1 <= M <= 65536."""
    from . import _lib as L
    from .loss import camera_intrinsics
    if not isinstance(d_nodes, torch.Tensor) or d_nodes.dim() != 3 or d_nodes.shape[2] != 3:
        raise L.RiggsHipError("node_semantic_labels: d_nodes must be (F, M, 3)")
    d_nodes = L.require_cuda_f32("d_nodes", d_nodes.detach())
    F, M = int(d_nodes.shape[0]), int(d_nodes.shape[1])
    cameras = list(cameras)
    if len(cameras) != F:
        raise L.RiggsHipError("node_semantic_labels: %d cameras for %d frames of d_nodes" % (len(cameras), F))
    if not (1 <= F <= L.CONSTANTS["RIGGS_SEMANTIC_MAX_FRAMES"] and 1 <= M <= L.CONSTANTS["RIGGS_SEMANTIC_MAX_NODES"]):
        raise L.RiggsHipError("node_semantic_labels: needs 1 <= F <= %d frames and 1 <= M <= %d nodes, got F = %d, M = %d"
                              % (L.CONSTANTS["RIGGS_SEMANTIC_MAX_FRAMES"], L.CONSTANTS["RIGGS_SEMANTIC_MAX_NODES"], F, M))
    dev = d_nodes.device
    words = L.CONSTANTS["RIGGS_SEMANTIC_CAMERA_WORDS"]  # the record of include/riggs_hip.h: 16 + 4 floats, H, W, the map's pointer
    views = torch.stack([torch.as_tensor(c.world_view_transform).detach().to(device=dev, dtype=torch.float32).reshape(4, 4)
                         for c in cameras]).cpu().numpy()
    table = np.zeros((F, words), dtype=np.uint32)
    maps = []  # (alive until the launch is enqueued: the caching allocator then keeps their memory for the stream)
    for f, cam in enumerate(cameras):
        H, W = int(cam.image_height), int(cam.image_width)
        if not (1 <= H < 2 ** 24 and 1 <= W < 2 ** 24):
            raise L.RiggsHipError("node_semantic_labels: camera %d: image of %d x %d" % (f, H, W))
        table[f, :16] = views[f].reshape(16).view(np.uint32)
        table[f, 16:20] = np.array(camera_intrinsics(cam), dtype=np.float32).view(np.uint32)
        table[f, 20:22] = (H, W)
        seg = getattr(cam, "semantic_seg", None)
        if seg is None:
            continue
        seg = torch.as_tensor(seg).detach()
        if tuple(seg.shape) != (H, W) or seg.is_floating_point() or seg.is_complex() or seg.dtype is torch.bool:
            raise L.RiggsHipError("node_semantic_labels: camera %d: semantic_seg must be an integer (%d, %d) map, got %s %s"
                                  % (f, H, W, tuple(seg.shape), seg.dtype))
        seg = seg.to(device=dev, dtype=torch.int32).contiguous()
        maps.append(seg)
        table[f, 22:24] = (seg.data_ptr() & 0xFFFFFFFF, seg.data_ptr() >> 32)
    table_dev = torch.from_numpy(table.view(np.int32)).to(dev)
    labels = torch.empty(F, M, dtype=torch.float32, device=dev)
    median = torch.empty(M, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().riggs_node_semantic_labels(F, M, d_nodes.data_ptr(), table_dev.data_ptr(), labels.data_ptr(), median.data_ptr(), L.stream_ptr()), "riggs_node_semantic_labels")
    del maps
    return labels, median


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
def precompute_deformations(deform, gaussians, fids, coverage=None, model_path=None, num_gs_sample=0, manually_key_frame=-1,
                            cameras=None, symmetry=False, sequence_chunk=None):
    """The trained stage 1 at every training frame, and the skeleton drawn from it.  ``deform``: a ``ControlNodeWarp`` (or a
    model holding one as ``.deform``); ``gaussians``: the stage-1 ``GaussianModel``; ``fids`` (F,): the training frames' times,
    visited in ascending order (``coverage`` (F,), the frames' mask areas, is given in the order of ``fids``).

    Returns ``(pretrain_deform_info, skeleton_tree_info, template_offsets)``: the stacked ``d_xyz`` (F, N, 3), ``d_nodes``
    (F, M, 3), ``d_rotation``, ``d_scaling`` and ``d_joints`` = ``d_nodes[:, joint_node_indices]``; ``joints``,
    ``parent_indices``, ``joint_node_indices``, ``template_idx`` (an index into the sorted frames).  As in the reference the
    template frame becomes the rest pose: its ``d_xyz`` — the template offsets — is ADDED to ``gaussians._xyz`` and subtracted
    from every frame's ``d_xyz``.  ``num_gs_sample > 10`` first thins the Gaussians (``sampling_and_prune``); ``model_path``:
    where ``skeleton_tree.npz`` and ``skeleton.obj`` are written.

    ``symmetry=True`` is the reference trainer's call (train_rig.py:226-231): ``obtain_skeleton_tree`` gets a label per node and
    runs the symmetry pass — with ``cameras`` (F objects in the order of ``fids``, see ``node_semantic_labels``) the median over
    the frames of the labels the nodes project onto, ``node_semantic_labels(d_nodes, cameras)[1]``, and ``nodes_semantic_label``
    (F, M) is returned in the first dict; without cameras an all-zero vector, what the reference passes for a dataset without
    semantic maps (which still pairs chains, by length alone).  The default ``symmetry=False`` passes None — no symmetry pass,
    which the reference's trainer never does; ``cameras`` alone changes nothing.

    ``sequence_chunk=None``: one ``forward`` per frame, as the reference.  An integer: the frames go through
    ``ControlNodeWarp.deform_sequence`` in chunks of that size — the scan of the control nodes once per chunk instead of once
    per frame; the results agree with the loop's to float32 rounding."""
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
    if cameras is not None:
        cameras = list(cameras)
        if len(cameras) != fids.shape[0]:
            raise ValueError("precompute_deformations: %d cameras for %d frames" % (len(cameras), fids.shape[0]))
        cameras = [cameras[int(i)] for i in order]
    xyz = gaussians.get_xyz.detach()
    stacks = {"d_xyz": [], "d_nodes": [], "d_rotation": [], "d_scaling": []}
    if sequence_chunk is None:
        for i in range(fids.shape[0]):
            d = warp(xyz, warp.expand_time(fids[i:i + 1]), feature=gaussians.feature, motion_mask=gaussians.motion_mask)
            for k in stacks:
                stacks[k].append(d[k].detach())
        info = {k: torch.stack(v) for k, v in stacks.items()}
    else:
        for c0 in range(0, fids.shape[0], max(1, int(sequence_chunk))):
            d = warp.deform_sequence(xyz, fids[c0:c0 + max(1, int(sequence_chunk))], gaussians.feature, gaussians.motion_mask)
            for k in stacks:
                stacks[k].append(d[k])
        info = {k: torch.cat(v) for k, v in stacks.items()}
    template_idx = select_key_frame(info["d_nodes"], coverage, manually_key_frame)
    seg_labels = None
    if symmetry and cameras is not None:
        info["nodes_semantic_label"], seg_labels = node_semantic_labels(info["d_nodes"], cameras)
    elif symmetry:
        seg_labels = torch.zeros(info["d_nodes"].shape[1], dtype=torch.int32, device=dev)
    joints, parent_indices, joint_node_indices = obtain_skeleton_tree(info["d_nodes"][template_idx], info["d_nodes"], seg_labels,
                                                                      symmetry=seg_labels is not None)
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
