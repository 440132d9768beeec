"""Stage-1 control-node deformation with the reference's names (/root/reference/utils/time_utils.py:770-1236
``ControlNodeWarp``): K nearest control nodes per Gaussian in (xyz, hyper) space, Gaussian-kernel weights, blend of the nodes'
translations / local-frame rotations / rotation and scale residuals — ONE HIP launch forward, five backward (csrc/cnode.hip)
instead of a KNN extension call, ~10 (N, K, ·) gathers, an einsum and autograd's replay of them.

Covered: the configuration the trainer ships (KNN weights; ``local_frame``, ``d_rot_as_res``, ``with_node_weight``, ``hyper_dim``
free) through the HIP kernels; ``pred_opacity`` / ``pred_color`` (two more blends with the same weights, torch ops on the
kernel's neighbour lists) and ``skinning=True`` (softmax of a per-Gaussian (N, M) feature instead of KNN weights: a dense
(N, M) x (M, 14) product, left to the GEMM library) as the reference defines them; ``node_trans_bias`` (the GUI's drag-to-edit
path, time_utils.py:1165-1213: an as-rigid-as-possible re-posing of the Gaussians around dragged nodes, under ``no_grad``) in
torch ops on top of the kernel's blend — it runs per mouse event, not per training step.  The node network
(``self.network``: nodes, t -> per-node attributes; 512-1024 rows, time_utils.py:990-1002) is a torch module supplied by the
caller; ``deform_sequence`` evaluates a whole time track over one cloud — one network call, one blend launch whose scan of the
nodes runs once per track (inference only).  Networks: ``riggs_amd.node_network.DeformNetwork`` (csrc/node_mlp.hip) for the
shipped flags, ``riggs_amd.hash_network.HashDeformNetwork`` (csrc/hashgrid.hip) with ``use_hash=True``, or any module
``(x, t) -> dict``.
No CPU / eager fallback.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from . import node_reg as NR
from .node_gaussians import NodeGaussians

LOCAL_FRAME, ROT_AS_RES = 1, 2


class _ControlNodeBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, feature, mask, nodes, radius_log, weight_logit, trans, rot, scale, local_rot, K, hyper, flags):
        N, M = x.shape[0], nodes.shape[0]
        dev = x.device
        f32 = dict(dtype=torch.float32, device=dev)
        d_xyz, d_rot, d_scale = torch.empty(N, 3, **f32), torch.empty(N, 4, **f32), torch.empty(N, 3, **f32)
        nn_idx = torch.empty(N, K, dtype=torch.int32, device=dev)
        nn_weight, nn_dist = torch.empty(N, K, **f32), torch.empty(N, K, **f32)
        fs = feature.shape[1] if feature is not None else 0
        L.check(L.lib().riggs_cnode_forward(N, M, K, hyper, fs, nodes.shape[1], flags, x.data_ptr(), L.ptr(feature), L.ptr(mask),
                                            nodes.data_ptr(), radius_log.data_ptr(), L.ptr(weight_logit), trans.data_ptr(),
                                            rot.data_ptr(), scale.data_ptr(), L.ptr(local_rot), d_xyz.data_ptr(),
                                            d_rot.data_ptr(), d_scale.data_ptr(), nn_idx.data_ptr(), nn_weight.data_ptr(),
                                            nn_dist.data_ptr(), L.stream_ptr()), "riggs_cnode_forward")
        ctx.save_for_backward(x, feature, mask, nodes, radius_log, weight_logit, trans, rot, scale, local_rot, nn_idx, nn_dist)
        ctx.cfg = (K, hyper, flags)
        ctx.mark_non_differentiable(nn_idx, nn_weight, nn_dist)
        ctx.set_materialize_grads(False)
        return d_xyz, d_rot, d_scale, nn_idx, nn_weight, nn_dist

    @staticmethod
    def backward(ctx, g_xyz, g_rot, g_scale, *_):
        x, feature, mask, nodes, radius_log, weight_logit, trans, rot, scale, local_rot, nn_idx, nn_dist = ctx.saved_tensors
        K, hyper, flags = ctx.cfg
        N, M = x.shape[0], nodes.shape[0]
        lib = L.lib()
        f32 = dict(dtype=torch.float32, device=x.device)
        c = lambda g: None if g is None else g.to(torch.float32).contiguous()  # noqa: E731
        g_xyz, g_rot, g_scale = c(g_xyz), c(g_rot), c(g_scale)
        need = ctx.needs_input_grad
        g_feature = torch.empty_like(feature) if (feature is not None and need[1]) else None
        g_mask = torch.empty_like(mask) if (mask is not None and need[2]) else None
        g_trans, g_nrot, g_nscale = torch.empty_like(trans), torch.empty_like(rot), torch.empty_like(scale)
        g_local = torch.empty_like(local_rot) if local_rot is not None else None
        g_radius = torch.empty_like(radius_log)
        g_weight = torch.empty_like(weight_logit) if weight_logit is not None else None
        g_hyper = torch.empty(M, hyper, **f32) if hyper > 0 else None
        ws = torch.empty(max(int(lib.riggs_cnode_backward_workspace_floats(N, M, K, hyper)), 1), **f32)
        fs = feature.shape[1] if feature is not None else 0
        L.check(lib.riggs_cnode_backward(N, M, K, hyper, fs, nodes.shape[1], flags, x.data_ptr(), L.ptr(feature), L.ptr(mask),
                                         nodes.data_ptr(), radius_log.data_ptr(), L.ptr(weight_logit), trans.data_ptr(),
                                         rot.data_ptr(), scale.data_ptr(), L.ptr(local_rot), nn_idx.data_ptr(), nn_dist.data_ptr(),
                                         L.ptr(g_xyz), L.ptr(g_rot), L.ptr(g_scale), L.ptr(g_feature), L.ptr(g_mask),
                                         g_trans.data_ptr(), g_nrot.data_ptr(), g_nscale.data_ptr(), L.ptr(g_local),
                                         g_radius.data_ptr(), L.ptr(g_weight), L.ptr(g_hyper), ws.data_ptr(), L.stream_ptr()),
                "riggs_cnode_backward")
        g_nodes = None
        if need[3]:
            g_nodes = torch.zeros_like(nodes)
            if hyper > 0:
                g_nodes[:, 3:3 + hyper] = g_hyper
        return (None, g_feature, g_mask, g_nodes, g_radius, g_weight, g_trans, g_nrot, g_nscale, g_local, None, None, None)


def _blend_inputs(x, feature, motion_mask, nodes, _node_radius, _node_weight, hyper_dim, local_frame, d_rot_as_res):
    """What the blend kernels take besides the nodes' attributes, checked: ``(x, feature or None, mask (N,) or None, nodes,
    radius, weight or None, hyper, flags)``."""
    x = L.require_cuda_f32("x", x.detach(), (x.shape[0], 3)).contiguous()
    nodes = L.require_cuda_f32("nodes", nodes).contiguous()
    M = nodes.shape[0]
    hyper = hyper_dim if (hyper_dim > 0 and feature is not None) else 0
    if feature is not None:
        feature = L.require_cuda_f32("feature", feature).contiguous()
        if hyper == 0:
            feature = None
    mask = None
    N = x.shape[0]
    if isinstance(motion_mask, torch.Tensor):
        if motion_mask.numel() == N:
            mask = L.require_cuda_f32("motion_mask", motion_mask).reshape(N).contiguous()
        elif motion_mask.numel() != 1 or float(motion_mask) != 1.0:
            raise NotImplementedError("motion_mask must be per Gaussian (N, 1) or 1")
    elif motion_mask is not None and float(motion_mask) != 1.0:
        raise NotImplementedError("motion_mask must be per Gaussian (N, 1) or 1")
    radius = L.require_cuda_f32("_node_radius", _node_radius, (M,)).contiguous()
    weight = L.require_cuda_f32("_node_weight", _node_weight).reshape(M).contiguous() if _node_weight is not None else None
    flags = (LOCAL_FRAME if local_frame else 0) | (ROT_AS_RES if d_rot_as_res else 0)
    return x, feature, mask, nodes, radius, weight, hyper, flags


def control_node_blend(x, feature, motion_mask, nodes, _node_radius, _node_weight, node_attrs, K=3, hyper_dim=0,
                       local_frame=False, d_rot_as_res=True):
    """The per-Gaussian part of ``ControlNodeWarp.forward`` (time_utils.py:1138-1191) given the nodes' attributes
    ``node_attrs = {'d_xyz', 'd_rotation', 'd_scaling', 'local_rotation'}``; returns the reference's dict (without ``d_nodes``)
    plus ``nn_idx`` (int32), ``nn_weight``, ``nn_dist`` of ``cal_nn_weight`` (:934-964)."""
    x, feature, mask, nodes, radius, weight, hyper, flags = _blend_inputs(x, feature, motion_mask, nodes, _node_radius, _node_weight,
                                                                          hyper_dim, local_frame, d_rot_as_res)
    M = nodes.shape[0]
    f = lambda name, t, w: L.require_cuda_f32(name, t, (M, w)).contiguous()  # noqa: E731
    trans, rot, scale = f("d_xyz", node_attrs["d_xyz"], 3), f("d_rotation", node_attrs["d_rotation"], 4), f("d_scaling", node_attrs["d_scaling"], 3)
    local_rot = f("local_rotation", node_attrs["local_rotation"], 4) if local_frame else None
    d_xyz, d_rot, d_scale, nn_idx, nn_weight, nn_dist = _ControlNodeBlend.apply(
        x, feature, mask, nodes, radius, weight, trans, rot, scale, local_rot, int(K), int(hyper), flags)
    return {"d_xyz": d_xyz, "d_rotation": d_rot, "d_scaling": d_scale, "d_opacity": None, "d_color": None,
            "nn_idx": nn_idx, "nn_weight": nn_weight, "nn_dist": nn_dist}


def sequence_pass_frames(M: int, flags: int = 0) -> int:
    """Frames the sequence kernel takes per pass (csrc/cnode.hip); 1: it has no passes."""
    return int(L.lib().riggs_cnode_sequence_pass_frames(int(M), int(flags)))


def control_node_blend_sequence(x, feature, motion_mask, nodes, _node_radius, _node_weight, node_attrs, K=3, hyper_dim=0,
                                local_frame=False, d_rot_as_res=True):
    """``control_node_blend`` for T frames over one cloud in ONE launch: ``node_attrs`` holds (T, M, c) tensors, the outputs
    ``d_xyz`` (T, N, 3), ``d_rotation`` (T, N, 4), ``d_scaling`` (T, N, 3) are frame-major (``out[k][f]`` is contiguous);
    ``nn_idx`` (int32), ``nn_weight``, ``nn_dist`` (N, K) do not depend on time and are written once — the scan over the nodes
    runs once per track, not once per frame.  Inference only: no graph, no backward."""
    with torch.no_grad():
        x, feature, mask, nodes, radius, weight, hyper, flags = _blend_inputs(x, feature, motion_mask, nodes.detach(), _node_radius.detach(),
                                                                              None if _node_weight is None else _node_weight.detach(),
                                                                              hyper_dim, local_frame, d_rot_as_res)
        N, M, K = x.shape[0], nodes.shape[0], int(K)
        T = int(node_attrs["d_xyz"].shape[0])
        def f(name, w):  # (the kernel reads the quaternion tables 16 bytes at a time)
            t = L.require_cuda_f32(name, node_attrs[name].detach(), (T, M, w)).contiguous()
            return t if t.data_ptr() % 16 == 0 else t.clone()
        trans, rot, scale = f("d_xyz", 3), f("d_rotation", 4), f("d_scaling", 3)
        local_rot = f("local_rotation", 4) if local_frame else None
        f32 = dict(dtype=torch.float32, device=x.device)
        d_xyz, d_rot, d_scale = torch.empty(T, N, 3, **f32), torch.empty(T, N, 4, **f32), torch.empty(T, N, 3, **f32)
        lists = torch.empty if T > 0 else torch.zeros  # (an empty track launches nothing)
        nn_idx = lists(N, K, dtype=torch.int32, device=x.device)
        nn_weight, nn_dist = lists(N, K, **f32), lists(N, K, **f32)
        fs = feature.shape[1] if feature is not None else 0
        L.check(L.lib().riggs_cnode_sequence_forward(N, M, T, K, hyper, fs, nodes.shape[1], flags, x.data_ptr(), L.ptr(feature),
                                                     L.ptr(mask), nodes.data_ptr(), radius.data_ptr(), L.ptr(weight), trans.data_ptr(),
                                                     rot.data_ptr(), scale.data_ptr(), L.ptr(local_rot), d_xyz.data_ptr(),
                                                     d_rot.data_ptr(), d_scale.data_ptr(), nn_idx.data_ptr(), nn_weight.data_ptr(),
                                                     nn_dist.data_ptr(), L.stream_ptr()), "riggs_cnode_sequence_forward")
    return {"d_xyz": d_xyz, "d_rotation": d_rot, "d_scaling": d_scale, "d_opacity": None, "d_color": None,
            "nn_idx": nn_idx, "nn_weight": nn_weight, "nn_dist": nn_dist}


def knn_weights_torch(x, feature, nodes, _node_radius, _node_weight, nn_idx, hyper_dim):
    """``cal_nn_weight`` (time_utils.py:934-964) as differentiable torch ops on GIVEN neighbour lists (the HIP kernel's): used
    where autograd has to see the weights themselves (the opacity / colour blends)."""
    idx = nn_idx.long()
    q, nd = x.detach(), nodes[..., :3].detach()
    if hyper_dim > 0 and feature is not None:
        q = torch.cat([q, feature[..., :hyper_dim]], dim=-1)
        nd = torch.cat([nd, nodes[..., 3:3 + hyper_dim]], dim=-1)
    d2 = ((q[:, None] - nd[idx]) ** 2).sum(-1)
    w = torch.exp(-d2 / (2 * torch.exp(_node_radius)[idx] ** 2))
    if _node_weight is not None:
        w = w * torch.sigmoid(_node_weight)[idx][..., 0]
    w = w + 1e-7
    return w / w.sum(dim=-1, keepdim=True)


def skinning_blend(feature, motion_mask, node_attrs, d_rot_as_res=True, pred_opacity=False, pred_color=False):
    """``ControlNodeWarp.forward`` with ``skinning=True`` (time_utils.py:934-938, 1160-1191, 1214-1225; ``local_frame`` off — the
    reference's einsum does not take the skinning weights): weights = softmax over ALL nodes of the per-Gaussian feature, every
    blend a dense (N, M) x (M, c) product."""
    w = torch.softmax(feature, dim=-1)
    rot_bias = torch.tensor([1.0, 0.0, 0.0, 0.0], device=feature.device)
    mm = motion_mask
    out = {"d_xyz": (w @ node_attrs["d_xyz"]) * mm, "d_scaling": (w @ node_attrs["d_scaling"]) * mm}
    if d_rot_as_res:
        out["d_rotation"] = (w @ node_attrs["d_rotation"]) * mm
    else:
        out["d_rotation"] = ((w @ (node_attrs["d_rotation"] + rot_bias)) - rot_bias) * mm + rot_bias
    out["d_opacity"] = (w @ node_attrs["d_opacity"]) * mm if pred_opacity else None
    out["d_color"] = (w @ node_attrs["d_color"]) * mm if pred_color else None
    out["nn_weight"], out["nn_idx"], out["nn_dist"] = w, torch.arange(w.shape[1], device=w.device), None
    return out


# ---- the editing path's geometry (all under no_grad; M nodes, a few hundred) -------------------------------------------------
def _quat_to_mat(q):
    """Rotation matrices of un-normalised (w, x, y, z) quaternions, scale 2 / |q|^2 (time_utils.py:115-132)."""
    w, a, b, c = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    rows = [1 - s * (b * b + c * c), s * (a * b - c * w), s * (a * c + b * w),
            s * (a * b + c * w), 1 - s * (a * a + c * c), s * (b * c - a * w),
            s * (a * c - b * w), s * (b * c + a * w), 1 - s * (a * a + b * b)]
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def _mat_to_quat(m):
    """(w, x, y, z) of rotation matrices: of the four algebraically equal candidates the one with the largest denominator
    (time_utils.py:146-205; no sign convention)."""
    sq = torch.stack([1.0 + m[..., 0, 0] + m[..., 1, 1] + m[..., 2, 2], 1.0 + m[..., 0, 0] - m[..., 1, 1] - m[..., 2, 2],
                      1.0 - m[..., 0, 0] + m[..., 1, 1] - m[..., 2, 2], 1.0 - m[..., 0, 0] - m[..., 1, 1] + m[..., 2, 2]], -1)
    qa = torch.where(sq > 0, sq.clamp_min(0).sqrt(), torch.zeros_like(sq))
    a, b, c = m[..., 2, 1] - m[..., 1, 2], m[..., 0, 2] - m[..., 2, 0], m[..., 1, 0] - m[..., 0, 1]
    e, f, g = m[..., 1, 0] + m[..., 0, 1], m[..., 0, 2] + m[..., 2, 0], m[..., 1, 2] + m[..., 2, 1]
    cand = torch.stack([torch.stack([qa[..., 0] ** 2, a, b, c], -1), torch.stack([a, qa[..., 1] ** 2, e, f], -1),
                        torch.stack([b, e, qa[..., 2] ** 2, g], -1), torch.stack([c, f, g, qa[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * qa[..., None].clamp_min(0.1))
    pick = qa.argmax(-1)
    return torch.gather(cand, -2, pick[..., None, None].expand(pick.shape + (1, 4))).squeeze(-2)


def _quat_mul(p, q):
    """Hamilton product, result with a non-negative real part (time_utils.py:99-113)."""
    pw, px, py, pz = p.unbind(-1)
    qw, qx, qy, qz = q.unbind(-1)
    r = torch.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], -1)
    return torch.where(r[..., :1] < 0, -r, r)


def _knn_sq(a, b, K, rows=32768):
    """The K nearest rows of ``b`` for every row of ``a`` by squared Euclidean distance, ascending (what the reference asks
    pytorch3d.ops.knn_points for); exact differences, in slabs of rows."""
    ds, ix = [], []
    for s0 in range(0, a.shape[0], rows):
        d = ((a[s0:s0 + rows, None, :] - b[None, :, :]) ** 2).sum(-1)
        dk, ik = d.topk(K, dim=1, largest=False, sorted=True)
        ds.append(dk)
        ix.append(ik)
    return torch.cat(ds), torch.cat(ix)


class StaticNodeNetwork(nn.Module):
    """``StaticNetwork(return_tensors=True)`` (time_utils.py:288-301): zero attributes for every node."""

    def forward(self, x, t, **kwargs):
        z3, z4 = torch.zeros_like(x), torch.zeros(x.shape[0], 4, dtype=x.dtype, device=x.device)
        return {"d_xyz": z3, "d_rotation": z4, "d_scaling": z3.clone(), "local_rotation": z4.clone(), "hidden": None,
                "d_opacity": None, "d_color": None}


class ControlNodeWarp(NodeGaussians, nn.Module):
    """``ControlNodeWarp`` (time_utils.py:770-1236) for the shipped configuration: parameters ``nodes`` (M, 3 + hyper_dim),
    ``_node_radius`` (M), ``_node_weight`` (M, 1) with the reference's names and activations; ``network`` is the node network
    (a torch module ``(nodes_xyz, t) -> dict``; default: the static one).  The stage-1 trainer's lifecycle (``init``,
    ``densify``, the node Gaussians, ``state_dict``) and node regularisers (``arap_loss`` / ``elastic_loss`` / ``acc_loss`` over
    csrc/node_reg.hip, no host synchronisation) have the reference's names and signatures."""

    def __init__(self, node_num=512, K=3, with_node_weight=True, local_frame=False, d_rot_as_res=True, hyper_dim=2, network=None,
                 pred_opacity=False, pred_color=False, skinning=False, is_blender=False, init_pcl=None, use_hash=False,
                 hash_time=False, enable_densify_prune=False, with_arap_loss=False, is_scene_static=False, **kwargs):
        super().__init__()
        if use_hash and not (network is not None and "bbox" in dict(network.named_buffers())):
            raise NotImplementedError("use_hash: this constructor builds no network itself — pass network=HashDeformNetwork(...) "
                                      "(riggs_amd.hash_network), or any module with a 'bbox' buffer")
        if skinning and local_frame:
            raise NotImplementedError("skinning with local_frame: the reference's own forward fails there (its einsum expects per-"
                                      "Gaussian neighbour lists, time_utils.py:1152)")
        self.name = "node"
        self.is_blender, self.use_hash, self.hash_time = is_blender, use_hash, hash_time
        self.enable_dp, self.is_scene_static = enable_densify_prune, is_scene_static
        self.skinning, self.pred_opacity, self.pred_color = bool(skinning), bool(pred_opacity), bool(pred_color)
        hyper_dim = 0 if skinning else hyper_dim  # "skinning should not be with hyper" (time_utils.py:782)
        self.K, self.with_node_weight, self.local_frame, self.d_rot_as_res, self.hyper_dim = K, with_node_weight, local_frame, d_rot_as_res, hyper_dim
        if with_arap_loss and not is_scene_static:  # (time_utils.py:790-795)
            self.lambda_arap_landmarks = [1e-4, 1e-4, 1e-5, 1e-5, 0]
            self.lambda_arap_steps = [0, 5000, 10000, 20000, 20001]
        else:
            self.lambda_arap_landmarks, self.lambda_arap_steps = [0], [0]
        self.network = network if (network is not None and not is_scene_static) else StaticNodeNetwork()
        self.register_buffer("inited", torch.tensor(False))
        self.nodes = nn.Parameter(torch.randn(node_num, 3 + hyper_dim))
        if not skinning:  # (time_utils.py:807-810)
            self._node_radius = nn.Parameter(torch.randn(node_num))
            if with_node_weight:
                self._node_weight = nn.Parameter(torch.zeros(node_num, 1))
        self.reg_loss = 0.
        if init_pcl is not None:
            self.init(None, init_pcl)
        self.nodes_color_visualization = torch.ones_like(self.nodes)
        self.cached_nn_weight = False
        self.nn_weight, self.nn_dist, self.nn_idxs = None, None, None

    def update(self, iteration):
        if hasattr(self.network, "update"):
            self.network.update(iteration)

    @property
    def param_names(self):
        if self.skinning:
            return ["nodes", "deform"]
        return ["nodes", "_node_radius", "_node_weight"] if self.with_node_weight else ["nodes", "_node_radius"]

    def load_state_dict(self, state_dict, strict=True):
        """Node parameters are assigned (re-created when the node count differs), ``gs_*`` entries go to the node Gaussians, the
        rest is loaded non-strictly (time_utils.py:844-865)."""
        state_dict = dict(state_dict)
        names = self.param_names
        for key in list(state_dict):
            if key in names:
                v = state_dict[key]
                if getattr(self, key).shape != v.shape:
                    print(f"Loading nodes mismatching the original setting: {getattr(self, key).shape} and {v.shape}")
                    setattr(self, key, nn.Parameter(v))
                else:
                    getattr(self, key).data = v
            elif key.startswith("gs_"):
                try:
                    getattr(self.as_gaussians, key[3:]).data = state_dict[key]
                except Exception:
                    print(f"Directly set as values for {key} when loading deform gaussians")
                    setattr(self.as_gaussians, key[3:], state_dict[key])
        for key in names:
            state_dict.pop(key, None)
        return super().load_state_dict(state_dict, strict=False)

    def init(self, opt, init_pcl, hyper_pcl=None, keep_all=False, force_init=False, as_gs_force_with_motion_mask=False,
             force_gs_keep_all=False, reset_bbox=True, *, start=None, **kwargs):
        """Nodes from the initial point cloud (time_utils.py:874-922): all of it (``keep_all``, or fewer points than nodes:
        new parameters, the optimizer must be set up again) or a farthest-point sample of it or of ``hyper_pcl`` (from a random
        start, or from index ``start`` for a run that can be repeated); radius log(0.1 scene range), weights 0; then the node
        Gaussians, set up for training with ``opt``."""
        from .gaussian_model import farthest_point_sample
        if bool(self.inited) and not force_init:
            return
        self.inited.data = torch.ones_like(self.inited)
        dev = init_pcl.device
        if self.use_hash and reset_bbox and hasattr(self.network, "bbox"):  # the hash grid's box (time_utils.py:895-896), no read-back
            self.network.bbox.data = torch.stack([init_pcl.min() - .1, init_pcl.max() + .1]).float().to(self.network.bbox.device)
        if keep_all or self.node_num > init_pcl.shape[0]:
            self.nodes = nn.Parameter(torch.cat([init_pcl.float(), 1e-2 * torch.ones(init_pcl.shape[0], self.hyper_dim, device=dev)], -1))
            init_nodes_idx = None
            print("Initialization with all pcl. Need to reset the optimizer.")
        else:
            pcl_to_samp = init_pcl if hyper_pcl is None else hyper_pcl
            first = {} if start is None else {"start": torch.as_tensor(start, dtype=torch.long).reshape(1)}
            init_nodes_idx = farthest_point_sample(pcl_to_samp.detach()[None], self.node_num, **first)[0]
            self.nodes.data = torch.cat([init_pcl[init_nodes_idx].float(), 1e-2 * torch.ones(self.node_num, self.hyper_dim, device=dev)], -1)
        scene_range = init_pcl.max() - init_pcl.min()
        if self.skinning:
            if "feature" in kwargs:
                radius = .1 * scene_range + 1e-7
                kwargs["feature"].data = -torch.log((init_pcl[:, None] - self.nodes[None, ..., :3]).square().sum(-1) / radius ** 2)
        else:
            radius = torch.log(.1 * scene_range + 1e-7) * torch.ones(self.node_num, device=dev)
            if keep_all or self.node_num > init_pcl.shape[0]:
                self._node_radius = nn.Parameter(radius)
                self._node_weight = nn.Parameter(torch.zeros_like(self.nodes[:, :1]))
            else:
                self._node_radius.data = radius
                self._node_weight.data = torch.zeros_like(self.nodes[:, :1])
        self.gs = None
        if force_gs_keep_all:
            self.init_gaussians(init_pcl=init_pcl, with_motion_mask=as_gs_force_with_motion_mask)
        else:
            self.init_gaussians(init_pcl=self.nodes[..., :3], with_motion_mask=as_gs_force_with_motion_mask)
        if opt is not None:
            self.as_gaussians.training_setup(opt)
        print(f"Control node initialized with {self.nodes.shape[0]} from {init_pcl.shape[0]} points.")
        return init_nodes_idx

    @torch.no_grad()
    def hyper_trajectories(self, x, motion_mask, time_num=16):
        """(N, 3 time_num) rows the nodes are sampled by (train_gui.py:1349-1357): every point's position at ``time_num`` times
        from 0 to 1, ``x + query_network(x, t_i)['d_xyz'] * motion_mask``, side by side.  One network call per time, as the
        reference makes them (the node network picks its workgroup shape by the row count)."""
        x = x.detach()
        t_samp = torch.linspace(0, 1, time_num).to(x.device)
        trans_samp = [self.query_network(x=x, t=t_samp[i:i + 1, None].expand_as(x[..., :1]))["d_xyz"] * motion_mask
                      for i in range(time_num)]
        return (torch.stack(trans_samp, dim=1) + x[:, None]).reshape(x.shape[0], -1)

    def downsample(self, opt, strategy="samp_hyper", with_dynamic_mask=False, start=None, **kwargs):
        """The step at ``iterations_node_sampling`` (train_gui.py:1334-1370): thin the node Gaussians to the control nodes.
        ``'direct'``: every node Gaussian becomes a node and the new node Gaussians share the old ones' parameters.
        ``'samp_hyper'``: ``node_num`` of them — all, or with ``with_dynamic_mask`` those whose motion mask exceeds 0.5 — are
        picked by a farthest-point sample of their trajectories (``hyper_trajectories``; from index ``start`` of the masked
        points, or a random one), the nodes are re-initialised from the picks, the new node Gaussians take the picked
        parameters and are set up for training with ``opt``.  ``kwargs`` go to ``init``.  Returns the picked indices into the
        masked points (``None`` for ``'direct'``).  Resetting the deformation model's optimizer and zeroing the gradients
        (train_gui.py:1346, 1372-1373) stay with the caller."""
        old = self.as_gaussians

        def take(pick):  # the new node Gaussians' appearance from the old ones'
            new = self.as_gaussians
            for name in ["_features_dc", "_features_rest", "_scaling", "_opacity", "_rotation"] + (["feature"] if new.fea_dim > 0 else []):
                setattr(new, name, nn.Parameter(pick(getattr(old, name))))
            return new

        if strategy == "direct":
            self.init(opt=opt, init_pcl=old.get_xyz, keep_all=True, force_init=True, reset_bbox=False, **kwargs)
            take(lambda p: p)
            return None
        if strategy != "samp_hyper":
            raise L.RiggsHipError("downsample: strategy is 'direct' or 'samp_hyper', got %r" % (strategy,))
        xyz = old.get_xyz
        hyper_pcl = self.hyper_trajectories(xyz, old.motion_mask)
        dynamic_mask = old.motion_mask[..., 0] > .5
        if not with_dynamic_mask:
            dynamic_mask = torch.ones_like(dynamic_mask)
        masked = int(dynamic_mask.sum()) if with_dynamic_mask else xyz.shape[0]
        if masked < self.node_num:
            raise L.RiggsHipError("downsample: %d points to sample %d nodes from" % (masked, self.node_num))
        idx = self.init(init_pcl=xyz[dynamic_mask], hyper_pcl=hyper_pcl[dynamic_mask], force_init=True, opt=opt, reset_bbox=False,
                        start=start, **kwargs)
        take(lambda p: p[dynamic_mask][idx]).training_setup(opt)
        return idx

    def cal_nn_weight(self, x, K=None, feature=None, nodes=None, gs_kernel=True, temperature=1.):
        """(time_utils.py:934-964) the K nearest nodes of every row of ``x`` in (xyz, hyper) space and their weights.  Used by
        ``cal_node_importance`` (once per densification); the per-step paths use the HIP kernels."""
        if self.skinning:
            return torch.softmax(feature, dim=-1), None, torch.arange(self.node_num, device=feature.device)
        if self.cached_nn_weight and self.nn_weight is not None:
            return self.nn_weight, self.nn_dist, self.nn_idxs
        if self.hyper_dim > 0 and feature is not None:
            x = torch.cat([x.detach(), feature[..., :self.hyper_dim]], dim=-1)
        K = self.K if K is None else K
        nodes = self.nodes[..., :3].detach() if nodes is None else nodes[..., :3]
        if feature is not None:
            nodes = torch.cat([nodes[..., :3].detach(), self.nodes[..., 3:]], dim=-1)
        nn_dist, nn_idxs = _knn_sq(x, nodes, K)
        if not gs_kernel:
            return torch.softmax(-nn_dist / temperature, dim=-1), nn_dist, nn_idxs
        nn_weight = torch.exp(-nn_dist / (2 * self.node_radius[nn_idxs] ** 2))
        if self.with_node_weight:
            nn_weight = nn_weight * self.node_weight[nn_idxs][..., 0]
        nn_weight = nn_weight + 1e-7
        nn_weight = nn_weight / nn_weight.sum(dim=-1, keepdim=True)
        if self.cached_nn_weight:
            self.nn_weight, self.nn_dist, self.nn_idxs = nn_weight, nn_dist, nn_idxs
        return nn_weight, nn_dist, nn_idxs

    @torch.no_grad()
    def cal_node_importance(self, x, K=None, weights=None, feature=None):
        """(time_utils.py:1270-1288) per node the weighted mean of its Gaussians' weights, their weighted mean position and the
        sum of weights."""
        if self.hyper_dim > 0:
            x = torch.cat([x, feature[..., :self.hyper_dim]], dim=-1)
        K = self.K if K is None else K
        nn_weight, _, nn_idxs = self.cal_nn_weight(x=x[..., :3], K=K, feature=feature)
        flat = nn_idxs.reshape(-1)
        weights = torch.ones_like(x[:, 0]) if weights is None else weights
        ww = nn_weight * weights[:, None]
        node_importance = torch.zeros_like(self.nodes[:, 0]).index_add_(0, flat, ww.reshape(-1))
        node_edge_count = torch.zeros_like(self.nodes[:, 0]).index_add_(0, flat, nn_weight.reshape(-1))
        xs = x[:, None].expand(*nn_weight.shape, x.shape[-1]).reshape(-1, x.shape[-1])
        avg_affected_x = torch.zeros_like(self.nodes).index_add_(0, flat, ww.reshape(-1, 1) * xs)
        avg_affected_x = avg_affected_x / node_importance[:, None]
        node_importance = node_importance / (node_edge_count + 1e-7)
        return node_importance, avg_affected_x, node_edge_count

    @torch.no_grad()
    def densify(self, max_grad, optimizer, x, x_grad, feature=None, K=None, use_gaussians_grad=False, force_dp=False):
        """(time_utils.py:1290-1383) add a node at the weighted mean position of the Gaussians of every node whose mean
        gradient norm exceeds ``max_grad``, drop nodes no Gaussian uses; the optimizer's 'nodes' group (``param_names`` order)
        and the node Gaussians follow."""
        if not self.enable_dp and not force_dp:
            return
        if not bool(self.inited):
            print("No need to densify nodes before initialization.")
            return
        if self.skinning:
            print("No need to densify for skinning type")
            return
        x_grad[x_grad.isnan()] = 0.
        K = self.K if K is None else K
        weights = x_grad.norm(dim=-1)
        node_avg_xgradnorm, node_avg_x, node_edge_count = self.cal_node_importance(x=x, K=K, weights=weights, feature=feature)
        if use_gaussians_grad or not hasattr(self, "nodes_accumulated_grad"):
            selected = torch.logical_and(node_avg_xgradnorm > max_grad, node_avg_x.isnan().logical_not().all(dim=-1))
        else:
            selected = self.nodes_accumulated_grad / self.denom > max_grad
            self.nodes_accumulated_grad.data = 0
            self.denom = 0
        self.nodes_color_visualization = torch.ones_like(self.nodes[..., :3])
        pruned = node_edge_count == 0
        if selected.sum() > 0 or pruned.sum() > 0:
            print(f"Add {selected.sum()} nodes and prune {pruned.sum()} nodes. ", end="")
        else:
            return
        names = self.param_names

        def surgery(make):
            for group in optimizer.param_groups:
                if group["name"] != "nodes":
                    continue
                for i, name in enumerate(names):
                    old = group["params"][i]
                    state = optimizer.state.get(old, None)
                    new = nn.Parameter(make(i, old.detach()).requires_grad_(True))
                    if state is not None:
                        state["exp_avg"] = make(i, state["exp_avg"], zeros=True)
                        state["exp_avg_sq"] = make(i, state["exp_avg_sq"], zeros=True)
                        del optimizer.state[old]
                        optimizer.state[new] = state
                    group["params"][i] = new
                    setattr(self, name, new)

        if selected.sum() > 0:
            new_nodes = node_avg_x[selected]
            ext = [new_nodes, self._node_radius[selected]] + ([self._node_weight[selected]] if self.with_node_weight else [])
            surgery(lambda i, t, zeros=False: torch.cat([t, torch.zeros_like(ext[i]) if zeros else ext[i]], 0))
            self.nodes_color_visualization = torch.cat([self.nodes_color_visualization, torch.ones_like(new_nodes[..., :3])], 0)
            self.nodes_color_visualization[-new_nodes.shape[0]:, 1:] = 0  # new nodes in red
        if pruned.shape[0] < self.nodes.shape[0]:
            pruned = torch.cat([pruned, torch.zeros(self.nodes.shape[0] - pruned.shape[0], dtype=pruned.dtype, device=pruned.device)])
        keep = ~pruned
        if pruned.sum() > 0:
            self.nodes_color_visualization = self.nodes_color_visualization[keep]
            surgery(lambda i, t, zeros=False: t[keep])
        if not self.with_node_weight:
            self._node_weight = torch.zeros_like(self.nodes[..., :1])
        # (_xyz aliases the old nodes[..., :3], a strided view; the row gathers want dense rows — it is re-aliased below)
        self.gs._xyz.data = self.gs._xyz.data.contiguous()
        self.gs.densify_and_split(selected_pts_mask=selected, N=1, without_prune=True)
        self.gs.prune_points(pruned)
        self.gs._xyz.data = self.nodes[..., :3]
        print(f"With {self.nodes.shape[0]} nodes left.")

    # ---- node regularisers (time_utils.py:1080-1120) over csrc/node_reg.hip: device random numbers, no host sync -----------
    def _t_center(self, t, delta_t):
        dev = self.nodes.device
        if t is None:
            return torch.rand((), device=dev)
        return t.squeeze() + delta_t * (torch.rand((), device=dev) - .5)

    def _nodes_at(self, t_samp):
        T = t_samp.shape[0]
        node_trans = self.node_deform(t=t_samp[None, :, None].expand(self.node_num, T, 1))["d_xyz"]
        return self.nodes[:, None, :3].detach() + node_trans  # M, T, 3

    def arap_loss(self, t=None, delta_t=0.05, t_samp_num=2):
        t = self._t_center(t, delta_t)
        nodes_t = self._nodes_at(torch.rand(t_samp_num, device=self.nodes.device) * delta_t + t - .5 * delta_t)
        nn_idx, _ = NR.connectivity_padded(nodes_t[:, 0].detach(), K=10)
        return NR.arap_error_padded(nodes_t.permute(1, 0, 2), nn_idx)

    def elastic_loss(self, t=None, delta_t=0.005, K=2, t_samp_num=8):
        t = self._t_center(t, delta_t)
        nodes_t = self._nodes_at(torch.rand(t_samp_num, device=self.nodes.device) * delta_t + t - .5 * delta_t)
        nn_idx, _ = NR.node_knn(self.nodes[:, :3 + self.hyper_dim].detach(), K + 1)
        w = NR.node_graph_weight(self.nodes, self._node_radius, self._node_weight if self.with_node_weight else None,
                                 self.hyper_dim, nn_idx)
        return NR.elastic_energy(nodes_t, nn_idx[:, 1:].contiguous(), w[:, 1:])

    def acc_loss(self, t=None, delta_t=.005):
        t = self._t_center(t, delta_t)
        return NR.acc_energy(self._nodes_at(torch.stack([t - delta_t, t, t + delta_t])))

    @property
    def node_radius(self):
        return torch.exp(self._node_radius)

    @property
    def node_weight(self):
        return torch.sigmoid(self._node_weight)

    @property
    def node_num(self):
        return self.nodes.shape[0]

    def trainable_parameters(self):
        if self.skinning:  # (time_utils.py:825-827)
            return [{"params": list(self.network.parameters()), "name": "deform"}, {"params": [self.nodes], "name": "nodes"}]
        node_params = [self.nodes, self._node_radius] + ([self._node_weight] if self.with_node_weight else [])
        return [{"params": list(self.network.parameters()), "name": "deform"}, {"params": node_params, "name": "nodes"}]

    def expand_time(self, t):
        return t.unsqueeze(0).expand(self.nodes.shape[0], -1)

    def query_network(self, x, t, **kwargs):
        return self.network(x=x, t=t, **kwargs)

    def node_deform(self, t, **kwargs):
        if t.dim() == 3:  # (M, T, 1): the nodes at T times each (time_utils.py:990-1002)
            M, T = t.shape[0], t.shape[1]
            x = self.nodes[:, None, :3].detach().expand(M, T, 3).reshape(-1, 3)
            v = self.network(x=x, t=t.reshape(-1, 1), **kwargs)
            return {k: (a.view(M, T, a.shape[-1]) if a is not None else None) for k, a in v.items()}
        return self.network(x=self.nodes[..., :3].detach(), t=t, **kwargs)

    # ---- the editing path (node_trans_bias): time_utils.py:1004-1011, 1044-1077, 969-988, 1122-1131, 1165-1213 -------------
    def get_trajectory(self, t_samp_num=8):
        t = torch.linspace(0, 1, t_samp_num, device=self.nodes.device)[None, :, None].expand(self.node_num, t_samp_num, 1)
        nd = self.node_deform(t=t)
        traj = self.nodes[:, None, :3].detach() + nd["d_xyz"]
        return traj.detach(), {k: (v[:, 0] if v is not None else None) for k, v in nd.items()}

    @torch.no_grad()
    def animation_tool(self, t, use_traj=True, t_samp_num=16):
        """The editor's drag tool over the nodes at time ``t`` (train_gui.py:204-223): a ``riggs_amd.arap.LapDeform`` whose
        neighbours are picked by the nodes' ``t_samp_num``-sample trajectory when ``use_traj`` is set, else by their positions at
        ``t``.  ``tool.deform_arap(handle_idx, handle_pos, return_R=True)[0] - tool.init_pcl`` is ``forward``'s ``node_trans_bias``."""
        from .arap import LapDeform
        t = torch.as_tensor(t, dtype=torch.float32, device=self.nodes.device).reshape(-1)[:1]
        nodes = self.nodes[..., :3].detach()
        pcl = nodes + self.node_deform(t=self.expand_time(t))["d_xyz"]
        trajectory = self.get_trajectory(t_samp_num=t_samp_num)[0] if use_traj else None
        return LapDeform(init_pcl=pcl, K=4, trajectory=trajectory, node_radius=self.node_radius.detach())

    def geodesic_distance_floyd(self, cur_node, K=8):
        """All-pairs shortest paths over the K-nearest-neighbour graph of the nodes (Floyd-Warshall on an (M, M) matrix)."""
        M = cur_node.shape[0]
        d2, idx = _knn_sq(cur_node, cur_node, K + 1)
        dist = torch.full((M, M), float("inf"), device=cur_node.device)
        dist.scatter_(1, idx, d2.sqrt())
        dist = torch.minimum(dist, dist.T)
        for i in range(M):
            dist = torch.minimum(dist[:, i, None] + dist[None, i, :], dist)
        return dist

    def cal_nn_weight_floyd(self, x, t0, cur_node, K=None, GraphK=2, temperature=1.0, cache_name="floyd", XisNode=False):
        """Weights of the K graph-nearest nodes of every point's nearest node; the graph distances are cached per name until
        the time moves by more than 1e-2 (time_utils.py:969-988)."""
        if not hasattr(self, cache_name + "_nn_dist") or (t0 is not None and (getattr(self, cache_name + "_t") - t0).abs().max() > 1e-2):
            gd, gi = self.geodesic_distance_floyd(cur_node=cur_node, K=GraphK).sort(dim=1)
            o = 1 if XisNode else 0
            setattr(self, cache_name + "_nn_dist", gd[:, o:K + o])
            setattr(self, cache_name + "_nn_idx", gi[:, o:K + o])
            if t0 is not None:
                setattr(self, cache_name + "_t", t0.clone())
        d2, i1 = _knn_sq(x, cur_node, 1)
        d2, i1 = d2[:, 0], i1[:, 0]
        kd = getattr(self, cache_name + "_nn_dist")[i1] + d2[:, None]
        return torch.softmax(-kd / temperature, dim=-1), kd, getattr(self, cache_name + "_nn_idx")[i1]

    def p2dR(self, p, p0=None, K=8, as_quat=True, mode="trajectory", t0=None):
        """Per node the rotation that best maps its edges to its K neighbours at rest (``p0``) onto the edges after the drag
        (``p``): Kabsch on weighted unit edges (time_utils.py:1044-1077).  Neighbours: K nearest by the nodes' trajectories
        (four time samples), by graph distance (``floyd``) or by rest position."""
        p = p.detach()
        nodes = self.nodes[..., :3].detach()
        t0_deform = None
        if mode == "trajectory":
            traj, t0_deform = self.get_trajectory(t_samp_num=4)
            base = traj[:, 0] if p0 is None else p0
            flat = traj.reshape(traj.shape[0], -1)
            d2, idx = _knn_sq(flat, flat, K + 1)
            d2, idx = d2[:, 1:], idx[:, 1:]
            w = torch.softmax(d2 / d2.mean(), dim=-1)
            edges = base[idx] - base[:, None]
        elif mode == "floyd":
            w, _, idx = self.cal_nn_weight_floyd(x=p, t0=t0, cur_node=p0, K=K + 1, GraphK=4, temperature=1e-1, cache_name="p2dR", XisNode=True)
            w, idx = w[:, 1:], idx[:, 1:]
            edges = p0[idx] - p0[:, None]
        else:
            d2, idx = _knn_sq(nodes, nodes, K + 1)
            d2, idx = d2[:, 1:], idx[:, 1:]
            w = torch.softmax(d2 / d2.mean(), dim=-1)
            base = nodes if p0 is None else p0
            edges = base[idx] - base[:, None]
        edges_t = p[idx] - p[:, None]
        edges = edges / (edges.norm(dim=-1, keepdim=True) + 1e-5)
        edges_t = edges_t / (edges_t.norm(dim=-1, keepdim=True) + 1e-5)
        S = torch.einsum("nka,nk,nkb->nab", edges, w, edges_t)
        U, _, Vh = torch.linalg.svd(S.cpu())  # (M, 3, 3): tiny, and the host's LAPACK is what torch.svd means everywhere
        dR = (Vh.transpose(-1, -2) @ U.transpose(-1, -2)).to(S.device)
        return (_mat_to_quat(dR) if as_quat else dR), t0_deform

    @torch.no_grad()
    def _edit(self, x, t, out, node_attrs, node_trans_bias, motion_mask):
        """The Gaussians re-posed around dragged nodes: every Gaussian keeps its offset to its (graph-)nearest nodes, rotated
        with them (time_utils.py:1165-1213).  ``out``: the blend without the drag."""
        rot_bias = torch.tensor([1.0, 0.0, 0.0, 0.0], device=x.device)
        node_trans = node_attrs["d_xyz"]
        cur_node = (self.nodes[..., :3] + node_trans).detach()
        nodes_t = cur_node + node_trans_bias
        gs_init = x + out["d_xyz"]
        if not self.d_rot_as_res:
            node_rot = node_attrs["d_rotation"]  # (already bias-multiplied by forward())
            d2, idx = _knn_sq(gs_init, cur_node, 32)
            w = torch.exp(-d2 / (2 * self.node_radius[idx] ** 2))
            if self.with_node_weight:
                w = w * self.node_weight[idx][..., 0]
            w = w + 1e-7
            w = w / w.sum(dim=-1, keepdim=True)
            R = _quat_to_mat(node_rot + rot_bias)[idx]
            gs_t = nodes_t[idx] + torch.einsum("gkab,gkb->gka", R, gs_init[:, None] - cur_node[idx])
            out["d_xyz"] = ((gs_t * w[..., None]).sum(dim=1) - x) * motion_mask
            return out
        w, _, idx = self.cal_nn_weight_floyd(x=gs_init, t0=t, cur_node=cur_node, K=8, GraphK=3, temperature=1e-3, XisNode=False)
        q_bias, _ = self.p2dR(p=nodes_t, p0=cur_node, K=8, as_quat=True, mode="trajectory", t0=t)
        R = _quat_to_mat(q_bias)[idx]
        gs_t = nodes_t[idx] + torch.einsum("gkab,gkb->gka", R, gs_init[:, None] - cur_node[idx])
        out["d_xyz"] = ((gs_t * w[..., None]).sum(dim=1) - x) * motion_mask
        out["d_rotation_bias"] = ((q_bias[idx] * w[..., None]).sum(dim=1) - rot_bias) * motion_mask + rot_bias
        return out

    @torch.no_grad()
    def deform_sequence(self, x, times, feature, motion_mask, animation_d_values=None, node_trans_bias=None, **kwargs):
        """``forward`` at every time of ``times`` (T,) over one cloud: ONE call of the node network for all T M rows and ONE
        blend launch (csrc/cnode.hip: cnode_sequence_kernel) in which every Gaussian finds its K nodes and their weights once
        — they do not depend on time — and then only gathers its nodes' records frame by frame.  Returns ``d_xyz`` (T, N, 3),
        ``d_rotation`` (T, N, 4), ``d_scaling`` (T, N, 3), ``d_nodes`` (T, M, 3), ``d_opacity`` / ``d_color`` (T, N, .) or None,
        ``nn_idx``, ``nn_weight``, ``nn_dist`` (N, K) and ``times``; frame-major, so ``out["d_xyz"][f]`` is contiguous and
        goes into ``render()`` as it is.  ``animation_d_values``: overrides of (T, M, c) per key, applied as ``forward`` applies
        its own; ``kwargs`` go to the network.

        INFERENCE ONLY: it runs under ``torch.no_grad()``, its outputs carry no graph, ``reg_loss`` and the module's training
        state are left alone.  ``node_trans_bias`` (the editing path) is per mouse event, not per track: not implemented."""
        if node_trans_bias is not None:
            raise NotImplementedError("deform_sequence: node_trans_bias (the editing path) works on one time; use forward()")
        times = torch.as_tensor(times, dtype=torch.float32, device=self.nodes.device)
        if times.dim() != 1:
            raise ValueError("deform_sequence: times must be (T,), got %s" % (tuple(times.shape),))
        T, M, N = int(times.shape[0]), self.node_num, int(x.shape[0])
        if T > 0:  # one network call for the T M rows, laid out frame-major for the kernel
            nd = self.node_deform(t=times[None, :, None].expand(M, T, 1), **kwargs)
            node_attrs = {k: v.transpose(0, 1).contiguous() for k, v in nd.items() if v is not None and k != "hidden"}
        else:
            z = lambda c: torch.zeros(0, M, c, device=self.nodes.device)  # noqa: E731
            node_attrs = {"d_xyz": z(3), "d_rotation": z(4), "d_scaling": z(3), "local_rotation": z(4), "d_opacity": z(1), "d_color": z(3)}
        if animation_d_values is not None:
            for k, v in animation_d_values.items():
                if v.dim() != 3 or v.shape[0] != T or v.shape[1] != M or (k in node_attrs and v.shape[2] != node_attrs[k].shape[2]):
                    raise ValueError("deform_sequence: animation_d_values[%r] has shape %s, expected (%d, %d, c)"
                                     % (k, tuple(v.shape), T, M))
                node_attrs[k] = v.detach()
        if self.skinning:  # the dense path: the softmax once, one batched product over the frames
            out = skinning_blend(feature.detach(), motion_mask, node_attrs, self.d_rot_as_res, self.pred_opacity, self.pred_color)
        else:
            nw = self._node_weight if self.with_node_weight else None
            out = control_node_blend_sequence(x, feature, motion_mask, self.nodes, self._node_radius, nw, node_attrs, K=self.K,
                                              hyper_dim=self.hyper_dim, local_frame=self.local_frame, d_rot_as_res=self.d_rot_as_res)
            idx = out["nn_idx"].long()
            for on, k in ((self.pred_opacity, "d_opacity"), (self.pred_color, "d_color")):  # (time_utils.py:1214-1225), all frames at once
                if on:
                    out[k] = (node_attrs[k][:, idx] * out["nn_weight"][None, :, :, None]).sum(dim=2) * motion_mask
        out["d_nodes"] = self.nodes[None, :, :3].detach() + node_attrs["d_xyz"]
        out["times"] = times
        return out

    def forward(self, x, t, feature, motion_mask, animation_d_values=None, node_trans_bias=None, iteration=0, is_training=True,
                **kwargs):
        if t.dim() == 0:
            t = self.expand_time(t)
        node_attrs = dict(self.node_deform(t=t))
        if animation_d_values is not None:
            node_attrs.update(animation_d_values)
        if node_trans_bias is not None:
            if self.skinning:
                raise NotImplementedError("node_trans_bias with skinning: the reference's own forward fails there (cal_nn_weight "
                                          "is asked for the weights of feature=None, time_utils.py:936)")
            if not self.d_rot_as_res:  # the dragged nodes' rotations enter the blend itself (time_utils.py:1165-1172)
                with torch.no_grad():
                    rb = torch.tensor([1.0, 0.0, 0.0, 0.0], device=x.device)
                    cur = (self.nodes[..., :3] + node_attrs["d_xyz"]).detach()
                    q_bias, _ = self.p2dR(p=cur + node_trans_bias, p0=cur, K=8, as_quat=True, mode="trajectory", t0=t)
                node_attrs["d_rotation"] = _quat_mul(q_bias, node_attrs["d_rotation"] + rb) - rb
        if self.skinning:
            out = skinning_blend(feature, motion_mask, node_attrs, self.d_rot_as_res, self.pred_opacity, self.pred_color)
        else:
            nw = self._node_weight if self.with_node_weight else None
            out = control_node_blend(x, feature, motion_mask, self.nodes, self._node_radius, nw, node_attrs, K=self.K,
                                     hyper_dim=self.hyper_dim, local_frame=self.local_frame, d_rot_as_res=self.d_rot_as_res)
            if self.pred_opacity or self.pred_color:  # (time_utils.py:1214-1225) the same weights, seen by autograd
                w = knn_weights_torch(x, feature, self.nodes, self._node_radius, nw, out["nn_idx"], self.hyper_dim)
                idx = out["nn_idx"].long()
                if self.pred_opacity:
                    out["d_opacity"] = (node_attrs["d_opacity"][idx] * w[..., None]).sum(dim=1) * motion_mask
                if self.pred_color:
                    out["d_color"] = (node_attrs["d_color"][idx] * w[..., None]).sum(dim=1) * motion_mask
        out["d_nodes"] = self.nodes[..., :3] + node_attrs["d_xyz"]
        if node_trans_bias is not None:
            out = self._edit(x.detach(), t, out, node_attrs, node_trans_bias, motion_mask)
        self.reg_loss = 0.
        lambda_arap = NR.landmark_interpolate(self.lambda_arap_landmarks, self.lambda_arap_steps, iteration)
        if self.training and lambda_arap > 0 and is_training:  # (time_utils.py:1229-1233)
            self.reg_loss = self.reg_loss + self.arap_loss() * lambda_arap
        return out
