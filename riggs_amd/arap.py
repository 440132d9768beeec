"""As-rigid-as-possible handle editing of the control nodes: the producer of ``ControlNodeWarp.forward(node_trans_bias=...)``.

  * ``ARAPDeformer``   the reference's utils/arap_deform.py: a graph over N nodes, and ``deform`` = "these M nodes go there" ->
                       positions (and rotations) of all N nodes (Sorkine & Alexa 2007: local rotation fits alternating with a
                       global linear solve, an initial solve plus ``iterations`` = 3 rounds)
  * ``LapDeform``      the reference's lap_deform.py: the editor's wrapper, radius = extent / 8 and K = 16
                       (``ControlNodeWarp.animation_tool`` builds one over the nodes at a time t)

Three time scales.  THE GRAPH is built once per object in torch ops (per session).  THE OPERATOR depends on which nodes are handles
and not on where they are: it is built when the set changes (a click), in float64, and cached on the object keyed by the set.  THE
DRAG (a mouse event) is one C call and one launch (csrc/arap.hip; include/riggs_hip.h states the method step by step,
tests/arap_ref.py restates it in NumPy): no read-back and no allocation that synchronises, so a second ``deform`` with the same
handle set and new positions in the same tensors replays inside a ``torch.cuda.graph``.

Two stated rules differ from the reference, each where the reference is ill-defined:

  1. Edge weights (``arap_graph``).  ``cal_connectivity_from_points`` takes the mean squared distance over ALL K columns; a dropped
     edge has distance inf, the mean is inf and every weight is exp(-d / inf) = 1 for a kept edge but exp(-inf / inf) = NaN for a
     dropped one, so one dropped edge makes the reference's weights NaN and its lstsq fail.  Here the mean is taken over the KEPT
     edges and a dropped edge has weight 0.  Where the reference drops no edge this is the reference's formula unchanged.
  2. The solve.  ``lstsq_with_handles`` is undefined where A_u (the non-handle columns of A = L_opt) is rank deficient.  Here every
     solve is ``x_u = p0_u + pinv(A_u) (b - A x_init)`` with ``x_init`` = the rest positions with the handles moved, and singular
     values below ``rcond`` times the largest are dropped (``null_dims`` counts them): a direction the handles do not determine
     keeps its rest position.  Where A_u has full rank this equals the reference's least-squares solution.

Limits: N <= 1024 nodes, K <= 16 neighbours, M >= 1 handles.  Out of scope: ``point_mask`` (the reference's dead
``mask_control_points`` branch: NotImplementedError), the trainable ``weight`` / optimizer, ``LapDeform.deform`` (the plain
Laplacian solve), ``energy`` and ``energy_arap``.  Inference only.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

__all__ = ["ARAPDeformer", "LapDeform", "arap_graph", "MAX_NODES", "MAX_K"]

MAX_NODES = L.CONSTANTS["RIGGS_ARAP_EDIT_MAX_NODES"]
MAX_K = L.CONSTANTS["RIGGS_ARAP_EDIT_MAX_K"]
LEAST_EDGE_NUM = 3  # cal_connectivity_from_points' default: a node's three nearest neighbours are kept whatever the radius


def arap_graph(points, radius, K, trajectory=None):
    """``cal_connectivity_from_points`` (utils/deform_utils.py:51-103) with ``adaptive_weighting=True``, lists kept padded:
    -> (nn_idx (N, K) int32 with -1 for a dropped edge, nn_dist (N, K) squared distances with inf there, weight (N, K)).

    Neighbours: the K nearest other nodes by squared distance between the rows of ``points`` (N, 3), or of ``trajectory``
    (N, T, 3) flattened and divided by T — a stable sort of the N x N distances, ties to the lowest index, the first column
    (the node itself) removed.  Columns from the fourth on are dropped where the distance is not below ``radius ** 2``.
    ``weight = exp(-d / mean) / row sum`` with the mean over the KEPT edges and 0 for a dropped edge: where no edge is dropped this
    is the reference's formula unchanged; where one is, the reference's mean is inf and its weights are NaN."""
    feat = points if trajectory is None else trajectory.reshape(trajectory.shape[0], -1) / trajectory.shape[1]
    feat = feat.detach().float()
    N = feat.shape[0]
    d = torch.zeros(N, N, dtype=torch.float32, device=feat.device)
    for c in range(feat.shape[1]):  # (sum of squared differences, coordinate by coordinate: no Gram-matrix cancellation)
        diff = feat[:, None, c] - feat[None, :, c]
        d = d + diff * diff
    nn_dist, nn_idx = torch.sort(d, dim=1, stable=True)
    nn_dist, nn_idx = nn_dist[:, 1:K + 1].contiguous(), nn_idx[:, 1:K + 1].contiguous()
    kept = torch.ones_like(nn_idx, dtype=torch.bool)
    kept[:, LEAST_EDGE_NUM:] = nn_dist[:, LEAST_EDGE_NUM:] < radius ** 2
    nn_idx = torch.where(kept, nn_idx, torch.full_like(nn_idx, -1))
    nn_dist = torch.where(kept, nn_dist, torch.full_like(nn_dist, float("inf")))
    mean = torch.where(kept, nn_dist, torch.zeros_like(nn_dist)).sum() / kept.sum()
    weight = torch.where(kept, torch.exp(-nn_dist / mean), torch.zeros_like(nn_dist))
    weight = weight / weight.sum(dim=-1, keepdim=True)
    return nn_idx.to(torch.int32), nn_dist, weight


def _handle_list(handle_idx):
    if isinstance(handle_idx, torch.Tensor):
        handle_idx = handle_idx.detach().cpu().numpy()
    h = np.asarray(handle_idx).reshape(-1)
    if h.size and not np.issubdtype(h.dtype, np.integer):
        raise ValueError("handle_idx must hold integers, got %s" % h.dtype)
    return tuple(int(v) for v in h)


class ARAPDeformer:
    """The reference's ``ARAPDeformer`` (utils/arap_deform.py:38-171).  ``verts`` (N, 3) float32; ``trajectory`` (N, T, 3) picks the
    neighbours by trajectory instead of by position.  ``node_radius`` is accepted and, as in the reference's default weighting,
    not used.  ``iterations`` is the reference's NUM_ITER; ``rcond`` the relative cutoff of the pseudo-inverse's singular values.

    ``verts``, ``K``, ``N``, ``radius``, ``weight`` (N, K), ``ii`` / ``jj`` / ``nn`` (the kept edges as the reference lists them)
    and ``nn_idx`` (N, K) int32 (the padded lists) are attributes; after a ``deform``, ``null_dims`` is the number of singular
    values the current handle set's operator dropped."""

    def __init__(self, verts, K=10, radius=0.3, point_mask=None, trajectory=None, node_radius=None, iterations=3, rcond=1e-6):
        if point_mask is not None:
            raise NotImplementedError("ARAPDeformer: point_mask belongs to the reference's dead mask_control_points branch")
        if verts.dim() != 2 or verts.shape[1] != 3:
            raise ValueError("ARAPDeformer: verts has shape %s, expected (N, 3)" % (tuple(verts.shape),))
        N, K = int(verts.shape[0]), int(K)
        if not 1 <= K <= MAX_K:
            raise ValueError("ARAPDeformer: K = %d, 1 to %d neighbours are supported" % (K, MAX_K))
        if not K + 1 <= N <= MAX_NODES:
            raise ValueError("ARAPDeformer: N = %d, K + 1 = %d to %d nodes are supported" % (N, K + 1, MAX_NODES))
        if trajectory is not None and (trajectory.dim() != 3 or trajectory.shape[0] != N):
            raise ValueError("ARAPDeformer: trajectory has shape %s, expected (%d, T, 3)" % (tuple(trajectory.shape), N))
        if int(iterations) < 0:
            raise ValueError("ARAPDeformer: iterations must not be negative")
        self.device = verts.device
        self.verts = verts.detach().float().contiguous()
        self.verts_copy = self.verts.clone()
        self.radius, self.K, self.N = radius, K, N
        self.iterations, self.rcond = int(iterations), float(rcond)
        self.point_mask = None
        self.nn_idx, self.nn_dist, self.weight = arap_graph(self.verts, radius, K, trajectory=None if trajectory is None else trajectory.detach())
        kept = self.nn_idx >= 0
        rows = torch.arange(N, device=self.device)[:, None].expand(N, K)
        cols = torch.arange(K, device=self.device)[None].expand(N, K)
        self.ii, self.jj, self.nn = rows[kept], self.nn_idx.long()[kept], cols[kept]
        self.null_dims = None
        self._operators = {}  # the handle set (sorted) -> (the operator (N, ld) float32, null_dims)
        self._handles = {}    # handle_idx as given (a tuple) -> its int32 device tensor
        self._last = None     # (the device tensor last given as handle_idx, its version, its tuple)

    def reset(self):
        self.verts = self.verts_copy.clone()

    # ---- per click -------------------------------------------------------------------------------------------------------------
    def laplacian(self, dtype=torch.float64):
        """A = L_opt (arap_deform.py:60-68): the identity with -weight on the kept edges."""
        A = torch.eye(self.N, dtype=dtype, device=self.device)
        A[self.ii, self.jj] = -self.weight[self.ii, self.nn].to(dtype)
        return A

    def operator(self, handle_idx):
        """-> (G, null_dims) for a handle set: G (N, ld) float32, ld = N rounded up to a multiple of 4 (the kernel reads 16 bytes
        at a time); the rows of the non-handle nodes are the rows of pinv(A_u), the handle rows and the columns >= N are zero.
        float64 SVD by torch.linalg, on the device where that works and else on the host; singular values <= rcond * the largest
        are dropped and counted.  Cached per set."""
        handles = self._check_handles(_handle_list(handle_idx))
        key = tuple(sorted(handles))
        if key not in self._operators:
            if len(self._operators) >= 16:
                self._operators.clear()
            A = self.laplacian()
            free = torch.ones(self.N, dtype=torch.bool, device=self.device)
            free[list(key)] = False
            Au = A[:, free]
            try:
                U, S, Vh = torch.linalg.svd(Au, full_matrices=False)
            except RuntimeError:  # (no float64 SVD on this device)
                U, S, Vh = (t.to(self.device) for t in torch.linalg.svd(Au.cpu(), full_matrices=False))
            keep = S > self.rcond * S.max()
            inv = torch.where(keep, 1.0 / torch.where(keep, S, torch.ones_like(S)), torch.zeros_like(S))
            pinv = (Vh.transpose(0, 1) * inv[None]) @ U.transpose(0, 1)  # (N - M, N)
            ld = (self.N + 3) // 4 * 4
            G = torch.zeros(self.N, ld, dtype=torch.float32, device=self.device)
            G[free, :self.N] = pinv.to(torch.float32)
            self._operators[key] = (G, int((~keep).sum()))
        return self._operators[key]

    def _check_handles(self, handles):
        if len(handles) == 0:
            raise ValueError("ARAPDeformer: the handle set is empty")
        if min(handles) < 0 or max(handles) >= self.N:
            raise ValueError("ARAPDeformer: a handle index is outside [0, %d)" % self.N)
        if len(set(handles)) != len(handles):
            raise ValueError("ARAPDeformer: a node is listed as a handle twice")
        return handles

    def _handles_of(self, handle_idx):
        """-> (the tuple, the int32 device tensor).  A device tensor that was the last call's, unchanged, is not read back."""
        if isinstance(handle_idx, torch.Tensor) and self._last is not None and self._last[0] is handle_idx \
                and self._last[1] == handle_idx._version:
            handles = self._last[2]
        else:
            handles = self._check_handles(_handle_list(handle_idx))
            self._last = (handle_idx, handle_idx._version, handles) if isinstance(handle_idx, torch.Tensor) else None
        if handles not in self._handles:
            if len(self._handles) >= 64:
                self._handles.clear()
            self._handles[handles] = torch.tensor(handles, dtype=torch.int32, device=self.device)
        return handles, self._handles[handles]

    # ---- per mouse event -------------------------------------------------------------------------------------------------------
    def _positions(self, name, p, shape):
        if not isinstance(p, torch.Tensor):
            p = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).to(self.device)
        p = L.require_cuda_f32(name, p.detach())
        if tuple(p.shape) != shape:
            raise ValueError("%s has shape %s, expected %s" % (name, tuple(p.shape), shape))
        return p

    def deform_batch(self, handle_idx, handle_pos, init_verts=None, return_R=False):
        """B independent drags of one handle set in one launch (the key-framed handle animation): ``handle_pos`` (B, M, 3),
        ``init_verts`` (B, N, 3) or None -> positions (B, N, 3), or with ``return_R`` (positions, quaternions (B, N, 4), None).
        Drag b's result is, bit for bit, what ``deform`` gives for it alone."""
        handles, h_dev = self._handles_of(handle_idx)
        M = len(handles)
        if not isinstance(handle_pos, torch.Tensor):
            handle_pos = np.asarray(handle_pos, dtype=np.float32)
        if len(handle_pos.shape) != 3:
            raise ValueError("handle_pos has shape %s, expected (B, %d, 3)" % (tuple(handle_pos.shape), M))
        B = int(handle_pos.shape[0])
        if B < 1:
            raise ValueError("deform_batch: no drag")
        handle_pos = self._positions("handle_pos", handle_pos, (B, M, 3))
        if init_verts is not None:
            init_verts = self._positions("init_verts", init_verts, (B, self.N, 3))
        verts = L.require_cuda_f32("verts", self.verts, (self.N, 3))
        G, self.null_dims = self.operator(handles)
        pos = torch.empty(B, self.N, 3, dtype=torch.float32, device=self.device)
        quat = torch.empty(B, self.N, 4, dtype=torch.float32, device=self.device) if return_R else None
        L.check(L.lib().riggs_arap_edit(B, self.N, self.K, M, verts.data_ptr(), self.nn_idx.data_ptr(), self.weight.data_ptr(),
                                        G.data_ptr(), int(G.shape[1]), h_dev.data_ptr(), handle_pos.data_ptr(), L.ptr(init_verts),
                                        self.iterations, pos.data_ptr(), L.ptr(quat), L.stream_ptr()), "riggs_arap_edit")
        return (pos, quat, None) if return_R else pos

    def deform(self, handle_idx, handle_pos, init_verts=None, return_R=False):
        """``handle_idx`` (M,) list, array or tensor; ``handle_pos`` (M, 3) array or tensor; ``init_verts`` (N, 3) replaces the
        initial solve -> positions (N, 3), or with ``return_R`` (positions, quaternions (N, 4) as (w, x, y, z), None)."""
        if not isinstance(handle_pos, torch.Tensor):
            handle_pos = np.asarray(handle_pos, dtype=np.float32)
        if len(handle_pos.shape) != 2:
            raise ValueError("handle_pos has shape %s, expected (M, 3)" % (tuple(handle_pos.shape),))
        out = self.deform_batch(handle_idx, handle_pos[None], None if init_verts is None else init_verts[None], return_R)
        return (out[0][0], out[1][0], None) if return_R else out[0]


class LapDeform:
    """The reference's ``LapDeform`` (lap_deform.py:96-224) as far as the editor's drag needs it: an ``ARAPDeformer`` over
    ``init_pcl`` with radius = the bounding box's diagonal / 8 and 16 neighbours (lap_deform.py:117-119).  ``K`` (the plain
    Laplacian's neighbour count) is kept as an attribute only: ``deform``, ``energy`` and ``energy_arap`` are out of scope."""

    def __init__(self, init_pcl, K=4, trajectory=None, node_radius=None):
        self.K, self.N = K, int(init_pcl.shape[0])
        self.init_pcl = init_pcl.detach().float().contiguous()
        self.init_pcl_copy = self.init_pcl.clone()
        radius = torch.linalg.norm(self.init_pcl.max(dim=0).values - self.init_pcl.min(dim=0).values) / 8
        self.arap_deformer = ARAPDeformer(self.init_pcl, radius=radius, K=16, trajectory=trajectory, node_radius=node_radius)

    def reset(self):
        self.init_pcl = self.init_pcl_copy.clone()
        self.arap_deformer.reset()

    def deform_arap(self, handle_idx, handle_pos, init_verts=None, return_R=False):
        """``ARAPDeformer.deform`` over ``init_pcl``; ``result[0] - init_pcl`` (with ``return_R=True``) is the ``node_trans_bias``
        of ``ControlNodeWarp.forward``."""
        return self.arap_deformer.deform(handle_idx, handle_pos, init_verts=init_verts, return_R=return_R)
