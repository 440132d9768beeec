"""Stage-1 node regularisers with the reference's names (utils/deform_utils.py:51-103, 123-198 and
utils/time_utils.py:1080-1120): the node-graph KNN, the ARAP energy of ``cal_arap_error``, the elastic and acceleration terms of
``ControlNodeWarp`` — over the HIP kernels of csrc/node_reg.hip.

The loss path keeps neighbour lists padded (M, K) int32 with -1 for dropped edges and never compacts them, draws its ARAP
sample rows with torch's device generator and returns device scalars: no host synchronisation in either direction.  The
backward passes are deterministic (no float atomics).  Neighbour indices and sample rows outside [0, M) count as dropped edges
in the kernels (never dereferenced).  ``cal_connectivity_from_points`` returns the reference's compacted
lists and may synchronise; the loss path does not call it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

ARAP_SAMPLE_NUM = 512
MAX_NODES, MAX_T, MAX_K = 8192, 16, 15


def _require_i32(name, t, shape):
    if not t.is_cuda:
        raise L.RiggsHipError("%s must be a CUDA(HIP) tensor — the product path is GPU-only" % name)
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape):
        raise L.RiggsHipError("%s must be int32 %s, got %s %s" % (name, tuple(shape), t.dtype, tuple(t.shape)))
    return t.contiguous()


def node_knn(points, Kq, drop_first=False, least_edge_num=0, radius=None):
    """For every row of ``points`` (M, D <= 16) the ``Kq`` <= 16 nearest rows by squared distance, ascending, ties to the lowest
    index (``pytorch3d.ops.knn_points(points, points, K=Kq)``); column 0 dropped when ``drop_first`` (the reference's
    ``[:, 1:]``, no special case for "self"); with ``radius``, columns >= ``least_edge_num`` whose distance is not below
    radius^2 become -1 (index) / inf (distance).  Returns int32 indices and float distances, (M, Kq - drop_first)."""
    pts = L.require_cuda_f32("points", points.detach()).contiguous()
    if pts.dim() != 2:
        raise L.RiggsHipError("points must be (M, D)")
    M, D = pts.shape
    ko = int(Kq) - int(bool(drop_first))
    idx = torch.empty(M, max(ko, 0), dtype=torch.int32, device=pts.device)
    dist = torch.empty(M, max(ko, 0), dtype=torch.float32, device=pts.device)
    r2 = float(np.float32(float(radius) ** 2)) if radius is not None else 0.0  # radius ** 2 compared in fp32, as torch does
    L.check(L.lib().riggs_node_knn(M, D, D, int(Kq), int(bool(drop_first)), int(least_edge_num), r2, pts.data_ptr(),
                                   idx.data_ptr(), dist.data_ptr(), L.stream_ptr()), "riggs_node_knn")
    return idx, dist


def connectivity_padded(points, radius=0.1, K=10, least_edge_num=3):
    """``cal_connectivity_from_points`` (mode 'nn', no trajectory) before compaction: (M, K) int32 neighbour lists with -1
    for edges beyond the radius, and their squared distances (inf there)."""
    return node_knn(points, K + 1, drop_first=True, least_edge_num=least_edge_num, radius=radius)


def cal_connectivity_from_points(points=None, radius=0.1, K=10, trajectory=None, least_edge_num=3, node_radius=None, mode="nn",
                                 GraphK=4, adaptive_weighting=True):
    """The reference's signature and results: compacted ``ii, jj, nn`` (int64) and the (M, K) edge weights (with a dropped edge
    anywhere the adaptive mean is inf and rows with a dropped edge hold NaN, as in the reference).  Synchronises (the
    compaction); the loss path uses ``connectivity_padded``."""
    if trajectory is not None or mode != "nn":
        raise NotImplementedError("cal_connectivity_from_points: only mode 'nn' without a trajectory")
    idx32, nn_dist = connectivity_padded(points, radius=radius, K=K, least_edge_num=least_edge_num)
    nn_idx = idx32.long()
    if adaptive_weighting:
        weight = torch.exp(-nn_dist / nn_dist.mean())
    elif node_radius is None:
        weight = torch.exp(-nn_dist)
    else:
        weight = torch.exp(-nn_dist / (2 * node_radius[nn_idx] ** 2))
    weight = weight / weight.sum(dim=-1, keepdim=True)
    Nv = nn_idx.shape[0]
    ii = torch.arange(Nv, device=nn_idx.device)[:, None].expand(Nv, K).reshape(-1)
    jj = nn_idx.reshape(-1)
    nn = torch.arange(K, device=nn_idx.device)[None].expand(Nv, K).reshape(-1)
    keep = jj != -1
    return ii[keep], jj[keep], nn[keep], weight


class _ArapEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seq, nn_idx, rows):
        T, M, _ = seq.shape
        K, Ns = nn_idx.shape[1], rows.shape[0]
        lib = L.lib()
        dev = seq.device
        rot = torch.empty(Ns, T, 9, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = torch.empty(int(lib.riggs_arap_workspace_floats(M, T, K, Ns)), dtype=torch.float32, device=dev)
        L.check(lib.riggs_arap_forward(M, T, K, Ns, seq.data_ptr(), nn_idx.data_ptr(), rows.data_ptr(), rot.data_ptr(),
                                       loss.data_ptr(), ws.data_ptr(), L.stream_ptr()), "riggs_arap_forward")
        ctx.save_for_backward(seq, nn_idx, rows, rot)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        seq, nn_idx, rows, rot = ctx.saved_tensors
        T, M, _ = seq.shape
        K, Ns = nn_idx.shape[1], rows.shape[0]
        lib = L.lib()
        g = g.reshape(1).to(torch.float32).contiguous()
        g_seq = torch.empty_like(seq)
        ws = torch.empty(int(lib.riggs_arap_workspace_floats(M, T, K, Ns)), dtype=torch.float32, device=seq.device)
        L.check(lib.riggs_arap_backward(M, T, K, Ns, seq.data_ptr(), nn_idx.data_ptr(), rows.data_ptr(), rot.data_ptr(),
                                        g.data_ptr(), g_seq.data_ptr(), ws.data_ptr(), L.stream_ptr()), "riggs_arap_backward")
        return g_seq, None, None


def arap_sample_rows(M, sample_num=ARAP_SAMPLE_NUM, device="cuda"):
    """``cal_arap_error``'s rows: all of them when M <= sample_num, else sample_num drawn uniformly with replacement (the
    distribution of ``np.random.choice(M, sample_num)``, from torch's device generator)."""
    if M > sample_num:
        return torch.randint(0, M, (sample_num,), device=device, dtype=torch.int32)
    return torch.arange(M, device=device, dtype=torch.int32)


def arap_error_padded(nodes_sequence, nn_idx, rows=None, sample_num=ARAP_SAMPLE_NUM):
    """``cal_arap_error`` with ``weight=None`` on padded (M, K) neighbour lists: nodes_sequence (T, M, 3), differentiable;
    the rotations are held constant in the backward pass (the reference estimates them under no_grad)."""
    seq = L.require_cuda_f32("nodes_sequence", nodes_sequence)
    if seq.dim() != 3 or seq.shape[2] != 3:
        raise L.RiggsHipError("nodes_sequence must be (T, M, 3)")
    T, M, _ = seq.shape
    nn_idx = _require_i32("nn_idx", nn_idx, (M, nn_idx.shape[1]))
    if rows is None:
        rows = arap_sample_rows(M, sample_num, seq.device)
    rows = _require_i32("rows", rows, (rows.shape[0],))
    return _ArapEnergy.apply(seq.contiguous(), nn_idx, rows)


def cal_arap_error(nodes_sequence, ii, jj, nn, K=10, weight=None, sample_num=ARAP_SAMPLE_NUM):
    """The reference's signature over compacted edge lists (binary edge weights, ``weight=None``)."""
    if weight is not None:
        raise NotImplementedError("cal_arap_error: only weight=None (binary edges), what arap_loss passes")
    M = nodes_sequence.shape[1]
    if ii.numel() and bool(((ii < 0) | (ii >= M) | (nn < 0) | (nn >= K)).any()):  # (a host sync: not the loss path)
        raise L.RiggsHipError("cal_arap_error: ii must lie in [0, M) and nn in [0, K)")
    nn_idx = torch.full((M, K), -1, dtype=torch.int32, device=nodes_sequence.device)
    nn_idx[ii, nn] = jj.to(torch.int32)
    return arap_error_padded(nodes_sequence, nn_idx, sample_num=sample_num)


class _ElasticEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nodes_t, nn_idx, weight):
        M, T, _ = nodes_t.shape
        K = nn_idx.shape[1]
        lib = L.lib()
        loss = torch.empty(1, dtype=torch.float32, device=nodes_t.device)
        ws = torch.empty(int(lib.riggs_elastic_workspace_floats(M, T, K)), dtype=torch.float32, device=nodes_t.device)
        L.check(lib.riggs_elastic_forward(M, T, K, nodes_t.data_ptr(), nn_idx.data_ptr(), weight.data_ptr(), loss.data_ptr(),
                                          ws.data_ptr(), L.stream_ptr()), "riggs_elastic_forward")
        ctx.save_for_backward(nodes_t, nn_idx, weight)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        nodes_t, nn_idx, weight = ctx.saved_tensors
        M, T, _ = nodes_t.shape
        K = nn_idx.shape[1]
        lib = L.lib()
        g = g.reshape(1).to(torch.float32).contiguous()
        g_x, g_w = torch.empty_like(nodes_t), torch.empty_like(weight)
        ws = torch.empty(int(lib.riggs_elastic_workspace_floats(M, T, K)), dtype=torch.float32, device=nodes_t.device)
        L.check(lib.riggs_elastic_backward(M, T, K, nodes_t.data_ptr(), nn_idx.data_ptr(), weight.data_ptr(), g.data_ptr(),
                                           g_x.data_ptr(), g_w.data_ptr(), ws.data_ptr(), L.stream_ptr()), "riggs_elastic_backward")
        return g_x, None, g_w


def elastic_energy(nodes_t, nn_idx, weight):
    """mean_m sum_k w_mk Var_t|n_t[j] - n_t[m]| / (Var.detach() + 1e-5) (time_utils.py:1091-1108, unbiased variance):
    nodes_t (M, T, 3), nn_idx (M, K) int32 (-1: no edge), weight (M, K); differentiable in nodes_t and weight."""
    x = L.require_cuda_f32("nodes_t", nodes_t)
    if x.dim() != 3 or x.shape[2] != 3:
        raise L.RiggsHipError("nodes_t must be (M, T, 3)")
    M = x.shape[0]
    nn_idx = _require_i32("nn_idx", nn_idx, (M, nn_idx.shape[1]))
    w = L.require_cuda_f32("weight", weight, (M, nn_idx.shape[1]))
    return _ElasticEnergy.apply(x.contiguous(), nn_idx, w.contiguous())


class _AccEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nodes_t):
        M = nodes_t.shape[0]
        lib = L.lib()
        loss = torch.empty(1, dtype=torch.float32, device=nodes_t.device)
        ws = torch.empty(int(lib.riggs_acc_workspace_floats(M)), dtype=torch.float32, device=nodes_t.device)
        L.check(lib.riggs_acc_forward(M, nodes_t.data_ptr(), loss.data_ptr(), ws.data_ptr(), L.stream_ptr()), "riggs_acc_forward")
        ctx.save_for_backward(nodes_t)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (nodes_t,) = ctx.saved_tensors
        g = g.reshape(1).to(torch.float32).contiguous()
        g_x = torch.empty_like(nodes_t)
        L.check(L.lib().riggs_acc_backward(nodes_t.shape[0], nodes_t.data_ptr(), g.data_ptr(), g_x.data_ptr(), L.stream_ptr()),
                "riggs_acc_backward")
        return g_x


def acc_energy(nodes_t):
    """mean_m |n0 + n2 - 2 n1| / (that.detach() + 1e-5) over nodes_t (M, 3, 3) (time_utils.py:1110-1120); the gradient of the
    norm at exactly zero is 0, as torch's."""
    x = L.require_cuda_f32("nodes_t", nodes_t, (nodes_t.shape[0], 3, 3))
    return _AccEnergy.apply(x.contiguous())


def node_graph_weight(nodes, radius_log, weight_logit, hyper_dim, nn_idx):
    """``cal_nn_weight(x=nodes[:, :3], feature=nodes[:, 3:], K)`` on given (M, K) neighbour lists (-1: none, weight 0) as
    differentiable torch ops: Gaussian kernel of the squared distance in (xyz detached, hyper) space, times the node weight,
    + 1e-7, normalised over the K columns.  Gradients reach the hyper coordinates (query and target), ``_node_radius`` and
    ``_node_weight``."""
    q = nodes[:, :3].detach()
    if hyper_dim > 0:
        q = torch.cat([q, nodes[:, 3:3 + hyper_dim]], dim=-1)
    valid = nn_idx >= 0
    idx = nn_idx.long().clamp_min(0)
    d2 = ((q[:, None] - q[idx]) ** 2).sum(-1)
    w = torch.exp(-d2 / (2 * torch.exp(radius_log)[idx] ** 2))
    if weight_logit is not None:
        w = w * torch.sigmoid(weight_logit)[idx][..., 0]
    w = torch.where(valid, w + 1e-7, torch.zeros_like(w))
    return w / w.sum(dim=-1, keepdim=True)


def landmark_interpolate(landmarks, steps, step):
    """The value of a piecewise log-linear schedule at ``step`` (utils/time_utils.py:485-503, 'log'): 0 before the first
    step, the last landmark (at least 0) from the last step on, 0 on a segment that ends at a non-positive landmark."""
    stage = int(sum(step >= s for s in steps))
    if stage == len(steps):
        return max(0, landmarks[-1])
    if stage == 0:
        return 0
    lo, hi = landmarks[stage - 1], landmarks[stage]
    if hi <= 0:
        return 0
    r = (step - steps[stage - 1]) / (steps[stage] - steps[stage - 1])
    return float(np.exp(np.log(lo) * (1 - r) + np.log(hi) * r))
