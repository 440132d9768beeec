"""Playing a trained rig back over a list of poses — what the reference's users do after training (render_rig.py's modes
``render_set`` / ``generate_random_motion`` / ``interpolate_time`` / ``interpolate_all``, the editor's "Motion Interpolation" panel,
interactive_GUI.py:1214-1256): key poses -> a pose track, the track skinned over ONE canonical cloud, and the colours of the
skinning-weight view.

Mirrors (same names, arguments, results) of
  * ``slerp_batch`` / ``run_interpolation``                          skeleton_utils/interpolation_utils.py:4-86
  * ``get_geometric_color`` / ``get_color_for_skinning_weights``     skeleton_utils/visualization.py:92-102, :125-129
and the additions ``SkeletonWarp.skinning_colors`` / ``SkeletonWarp.deform_sequence`` (implemented here, bound in
riggs_amd/skeleton.py) and ``render_sequence``.  Everything that depends on the canonical cloud alone — bone distances, the top-K
selection, the WeightMLP head, the skin colours — is computed once per track; per pose only the J transforms change
(csrc/deform.hip: lbs_sequence_kernel, skinning_colors_kernel; csrc/playback.hip: pose_slerp_kernel).  Inference only.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .skeleton import _mask_tensor, _zero_scaling

__all__ = ["slerp_batch", "run_interpolation", "get_geometric_color", "get_color_for_skinning_weights", "skinning_colors",
           "deform_sequence", "render_sequence", "sequence_pass_frames", "render_time_sequence"]


# --------------------------------------------------------------------------- key poses -> a pose track
def _slerp_launch(S, m, n, q0, q1, q_stride, t, tr0, tr1, strides, out_rot, out_trans):
    L.check(L.lib().riggs_pose_slerp(S, m, n, q0.data_ptr(), q1.data_ptr(), q_stride, t.data_ptr(), L.ptr(tr0), L.ptr(tr1),
                                     strides[0], strides[1], strides[2], out_rot.data_ptr(), L.ptr(out_trans), L.stream_ptr()),
            "riggs_pose_slerp")


def slerp_batch(q0, q1, t):
    """interpolation_utils.py:4-54: ``q0``, ``q1`` (n, 4) and ``t`` (m,) -> (n, m, 4) unit quaternions.  Step for step the
    reference: both inputs normalised, ``q1`` negated where the dot product is negative, the clamp, ``acos``, the ``sin`` weights —
    the linear ones where ``sin(theta_0) <= 1e-6`` — and the result normalised.  CUDA float32; ``t`` is used as it is given."""
    n, m = int(q0.shape[0]), int(t.shape[0])
    q0 = L.require_cuda_f32("q0", q0.detach(), (n, 4))
    q1 = L.require_cuda_f32("q1", q1.detach(), (n, 4))
    t = L.require_cuda_f32("t", t.detach(), (m,))
    out = torch.empty(n, m, 4, dtype=torch.float32, device=q0.device)
    _slerp_launch(1, m, n, q0, q1, 0, t, None, None, (0, 4, 4 * m), out, None)
    return out


def run_interpolation(key_poses, device, num_frames=20):
    """interpolation_utils.py:58-86: the editor's saved key poses -> ``num_frames`` poses per pair of neighbours
    (``t = linspace(0, 1, num_frames + 1)[:-1]``: a segment starts on its first key pose and stops short of its second), the
    segments one after another.  ``None`` for fewer than two key poses.  One launch for all segments, rotations and translations.

    A quirk of the reference: ``run_interpolation`` reads and writes the key ``'local_rotation2'``, while its own editor stores the
    key poses under ``'local_rotation'`` and reads ``'local_rotation'`` back from the result (interactive_GUI.py:403, :1217).
    Here a key pose is read from ``'local_rotation2'`` when it has one, else from ``'local_rotation'``, and the track is returned
    under BOTH names (the same tensor), so either caller finds it."""
    if len(key_poses) <= 1:
        print("Not enough key poses: #poses=", len(key_poses))
        return None
    m = int(num_frames)
    t = torch.linspace(0, 1, steps=m + 1)[:-1].to(device)
    rot = torch.stack([(p["local_rotation2"] if "local_rotation2" in p else p["local_rotation"]).detach().to(device).reshape(-1, 4)
                       for p in key_poses]).float().contiguous()
    tr = torch.stack([p["global_trans"].detach().to(device).reshape(-1)[:3] for p in key_poses]).float().contiguous()
    P, J = int(rot.shape[0]), int(rot.shape[1])
    S = P - 1
    new_poses = torch.empty(S * m, J, 4, dtype=torch.float32, device=rot.device)
    new_trans = torch.empty(S * m, 3, dtype=torch.float32, device=rot.device)
    L.require_cuda_f32("key poses", rot)
    # (segment s: key pose s -> key pose s + 1 of the stacked array)
    _slerp_launch(S, m, J, rot, rot[1:], 4 * J, t, tr, tr[1:], (m * J * 4, J * 4, 4), new_poses, new_trans)
    return {"local_rotation2": new_poses, "local_rotation": new_poses, "global_trans": new_trans, "num": new_poses.shape[0]}


# --------------------------------------------------------------------------- colours
def get_geometric_color(points):
    """visualization.py:92-102: a point's position inside the bounding box as a colour quantised to 1/255 steps — the reference's
    IEEE divisions and its multiplication each rounded on their own (separate elementwise kernels: nothing to contract),
    truncation by ``.int()``, ``>= 1 -> 0.99``, ``< 0 -> 0``.  (The divisor 255 is a device tensor: a division by a Python scalar
    becomes a multiplication by the reciprocal on the device, which rounds some steps differently.)"""
    max_p = points.max(0).values
    min_p = points.min(0).values
    scale = max_p - min_p
    new_points = (points - min_p) / scale
    point_colors = (new_points * 255).int() / torch.full((), 255.0, dtype=points.dtype, device=points.device)
    point_colors[point_colors >= 1] = 0.99
    point_colors[point_colors < 0] = 0
    return point_colors


def get_color_for_skinning_weights(points, vn_idx, vn_weight, control_points):
    """visualization.py:125-129, as the reference writes it (torch ops over the materialised weights: the form
    ``SkeletonWarp.skinning_colors`` replaces)."""
    node_colors = get_geometric_color(control_points)
    vn_colors = torch.index_select(node_colors, 0, vn_idx.reshape(-1)).reshape(points.shape[0], vn_weight.shape[1], 3)
    return torch.sum(vn_weight.unsqueeze(-1) * vn_colors, dim=1)


def _head_weight_mod(sw, x):
    """sigmoid(WeightMLP(x)) (skeleton_warp.py:56-61) or None — evaluated once per track; raises like ``deform_by_pose``."""
    if not sw.use_skinning_weight_mlp:
        return None
    if sw.K > 0:
        raise NotImplementedError("use_skinning_weight_mlp with K > 0: the reference gathers the MLP output with the 1-based bone "
                                  "indices (skeleton_warp.py:59), which runs off its (N, J-1) columns; only K = -1 is well defined")
    return L.require_cuda_f32("skinning weight offsets", sw._head_weight(x).detach(), (x.shape[0], sw.nodes.shape[0] - 1))


_MODES = {"blend": 0, "segment": 1}


def skinning_colors(sw, x, mode="blend", _weight_mod=None):
    """``SkeletonWarp.skinning_colors``: the (N, 3) colours of the skinning-weight view in one launch that computes a Gaussian's
    weights exactly as the skinning forward does (shared device code: all bones or the top-K set with its tie-breaking,
    ``weight_mod`` with the WeightMLP head on, bone k <-> child joint k + 1) and folds them on the spot; ``nn_weight`` / ``nn_idx``
    are never written.  ``"blend"``: ``sum_k w_k colour[k + 1]`` (``get_color_for_skinning_weights``); ``"segment"``: the colour of
    the largest weight, the first bone on equality (visualization.py:118-120).  The colours do not depend on the pose."""
    if mode not in _MODES:
        raise ValueError("mode must be 'blend' or 'segment', got %r" % (mode,))
    with torch.no_grad():
        sw._emb_cache = None
        x = L.require_cuda_f32("x", x.detach(), (x.shape[0], 3))
        joints = sw._joints()
        N, J = int(x.shape[0]), int(joints.shape[0])
        wm = _head_weight_mod(sw, x) if _weight_mod is None else _weight_mod  # (render_sequence hands the head's output over)
        sw._emb_cache = None
        node_colors = get_geometric_color(joints).contiguous()
        out = torch.empty(N, 3, dtype=torch.float32, device=x.device)
        rho = L.require_cuda_f32("_node_radius", sw._node_radius.detach(), (J,))
        L.check(L.lib().riggs_skinning_colors(N, J, sw.K, x.data_ptr(), joints.data_ptr(), sw._parents_dev(x.device).data_ptr(),
                                              rho.data_ptr(), L.ptr(wm), node_colors.data_ptr(), _MODES[mode], out.data_ptr(),
                                              L.stream_ptr()), "riggs_skinning_colors")
    return out


# --------------------------------------------------------------------------- a pose track over one cloud
def sequence_pass_frames(J: int, K: int = -1) -> int:
    """Frames the sequence kernel takes per pass at this joint count (csrc/deform.hip: seq_pass_frames)."""
    return int(L.lib().riggs_lbs_sequence_pass_frames(int(J), int(K)))


def _track(poses, J, device):
    """``poses`` -> (local_rot (M, J, 4), global_trans (M, 3) or (3,), its stride in floats)."""
    if isinstance(poses, dict):
        lr = poses["local_rotation"] if "local_rotation" in poses else poses["local_rotation2"]
        gt = poses["global_trans"]
    else:  # a list of node_attrs dicts (render_rig.py:278-303)
        lr = torch.stack([p["local_rotation"].reshape(-1, 4) for p in poses])
        gt = torch.stack([p["global_trans"].reshape(-1)[:3] for p in poses])
    lr = L.require_cuda_f32("local_rotation", lr.detach().to(device), (None, J, 4))
    M = int(lr.shape[0])
    gt = gt.detach().to(device)
    if gt.numel() == 3:  # one translation for the track
        gt, stride = gt.reshape(3), 0
    elif gt.numel() == 3 * M:
        gt, stride = gt.reshape(M, 3), 3
    else:
        raise L.RiggsHipError("global_trans has shape %s, expected (M, 3), (M, 1, 3) or (1, 3) with M = %d" % (tuple(gt.shape), M))
    return lr, L.require_cuda_f32("global_trans", gt), stride


def deform_sequence(sw, x, poses, motion_mask, _weight_mod=None):
    """``SkeletonWarp.deform_sequence``: ``deform_by_pose`` for a whole pose track in two launches.  ``poses``: a dict with
    ``'local_rotation'`` (M, J, 4) and ``'global_trans'`` (M, 3), (M, 1, 3) or one (1, 3) for all frames — what ``run_interpolation``
    returns — or a list of ``node_attrs`` dicts.  Returns ``d_xyz`` (M, N, 3), ``d_rotation`` (M, N, 4), ``d_nodes`` (M, J, 3),
    ``d_scaling`` (one shared zero (N, 3)), ``local_rotation``, ``global_trans``; frame-major, so ``out["d_xyz"][f]`` is contiguous
    and goes into ``render()`` as it is.

    INFERENCE ONLY: it runs as under ``torch.no_grad()``, its outputs carry no graph and nothing here has a backward.  The
    WeightMLP head (``use_skinning_weight_mlp``) is evaluated once for the track; the pose-dependent DeformMLP
    (``use_template_offsets``) once per frame, its offsets joining ``d_xyz[f]`` before the mask (skeleton_warp.py:152-158).  The
    module's per-call state (``skinning_weight_offsets``, ``template_offsets``) is left as it was."""
    with torch.no_grad():
        sw._emb_cache = None
        x = L.require_cuda_f32("x", x.detach(), (x.shape[0], 3))
        joints = sw._joints()
        N, J = int(x.shape[0]), int(joints.shape[0])
        lr, gt, gt_stride = _track(poses, J, x.device)
        M = int(lr.shape[0])
        mask = _mask_tensor(motion_mask, N, x.device)
        mflat = None if mask is None else L.require_cuda_f32("motion_mask", mask.detach().reshape(-1), (N,))
        wm = _head_weight_mod(sw, x) if _weight_mod is None else _weight_mod
        f32 = dict(dtype=torch.float32, device=x.device)
        transforms, node_rot, d_nodes = torch.empty(M, J, 12, **f32), torch.empty(M, J, 4, **f32), torch.empty(M, J, 3, **f32)
        d_xyz, d_rot = torch.empty(M, N, 3, **f32), torch.empty(M, N, 4, **f32)
        rho = L.require_cuda_f32("_node_radius", sw._node_radius.detach(), (J,))
        L.check(L.lib().riggs_lbs_sequence_forward(N, M, J, sw.K, x.data_ptr(), joints.data_ptr(), sw._parents_dev(x.device).data_ptr(),
                                                   rho.data_ptr(), lr.data_ptr(), gt.data_ptr(), gt_stride, L.ptr(mflat), L.ptr(wm),
                                                   transforms.data_ptr(), node_rot.data_ptr(), d_nodes.data_ptr(), d_xyz.data_ptr(),
                                                   d_rot.data_ptr(), L.stream_ptr()), "riggs_lbs_sequence_forward")
        if sw.use_template_offsets:
            m3 = None if mflat is None else mflat[:, None]
            for f in range(M):
                off = sw._head_detail(x, lr[f].reshape(-1)[None].expand(N, -1))
                d_xyz[f] += off if m3 is None else off * m3
        sw._emb_cache = None
        zs = _zero_scaling(sw, N, x.device)
    return {"d_xyz": d_xyz, "d_rotation": d_rot, "d_scaling": zs, "d_nodes": d_nodes, "local_rotation": lr, "global_trans": gt}


def render_sequence(viewpoint_camera, pc, sw, pipe, bg_color, poses, motion_mask=None, skinning=False, chunk=32,
                    d_rot_as_res=True):
    """A generator over the frames of a pose track: yields ``(pkg, skin_pkg_or_None, d_nodes[f])`` per pose, where ``pkg`` is
    ``render(camera, pc, pipe, bg_color, d_xyz[f], d_rotation[f], d_scaling, keep_lists=skinning)`` and — with ``skinning=True`` —
    ``skin_pkg`` the same frame recoloured by the skinning weights over ``pkg``'s tile lists (``render(..., override_color=colours,
    lists=pkg.lists)``: no second projection, sort or binning).  ``chunk`` poses are skinned per ``deform_sequence`` call, which
    bounds the (chunk, N, 7) buffers; the skin colours are computed once.  ``viewpoint_camera``: one camera, or a list of one per
    pose (``interpolate_all`` moves the camera with the pose).  ``motion_mask=None``: no mask, as in ``deform_by_pose``."""
    from .render import render
    x = pc.get_xyz.detach()
    lr, gt, gt_stride = _track(poses, int(sw.nodes.shape[0]), x.device)
    M = int(lr.shape[0])
    cams = list(viewpoint_camera) if isinstance(viewpoint_camera, (list, tuple)) else None
    if cams is not None and len(cams) != M:
        raise ValueError("render_sequence: %d cameras for %d poses" % (len(cams), M))
    chunk = max(1, int(chunk))
    with torch.no_grad():  # the WeightMLP head once for the colours and every chunk
        sw._emb_cache = None
        wm = _head_weight_mod(sw, x)
        sw._emb_cache = None
    colours = skinning_colors(sw, x, "blend", _weight_mod=wm) if skinning else None
    for c0 in range(0, M, chunk):
        c1 = min(M, c0 + chunk)
        seq = deform_sequence(sw, x, {"local_rotation": lr[c0:c1], "global_trans": gt[c0:c1] if gt_stride else gt}, motion_mask,
                              _weight_mod=wm)
        for f in range(c1 - c0):
            cam = viewpoint_camera if cams is None else cams[c0 + f]
            args = (cam, pc, pipe, bg_color, seq["d_xyz"][f], seq["d_rotation"][f], seq["d_scaling"])
            pkg = render(*args, d_rot_as_res=d_rot_as_res, keep_lists=bool(skinning))
            skin = render(*args, d_rot_as_res=d_rot_as_res, override_color=colours, lists=pkg.lists) if skinning else None
            yield pkg, skin, seq["d_nodes"][f]


# --------------------------------------------------------------------------- stage 1: a time track over one cloud
def render_time_sequence(viewpoint_camera, pc, warp, pipe, bg_color, times, chunk=32):
    """Stage-1 playback (the reference's render.py modes ``render_set`` / ``interpolate_time`` / ``interpolate_all``,
    render.py:100-116, :157-235): a generator over ``times`` (T,) that yields ``(pkg, d_nodes[f])`` per time, where ``pkg`` is
    ``render(camera, pc, pipe, bg_color, d_xyz[f], d_rotation[f], d_scaling[f], d_opacity=, d_color=, d_rot_as_res=warp.d_rot_as_res)``
    on the frames of ``ControlNodeWarp.deform_sequence``: ``chunk`` times per call, which bounds the (chunk, N, 10) buffers; the
    scan of the control nodes runs once per chunk, not once per frame.  ``viewpoint_camera``: one camera, or a list of one per
    time (``interpolate_all`` moves the camera with the time).  ``warp``: a ``ControlNodeWarp`` or a model holding one as
    ``.deform``.  With ``pc.use_isotropic_gs`` the rotation and scale residuals are zeroed (render.py:112-114).  Inference only."""
    from .render import render
    warp = getattr(warp, "deform", warp)
    x = pc.get_xyz.detach()
    times = torch.as_tensor(times, dtype=torch.float32, device=x.device)
    if times.dim() != 1:
        raise ValueError("render_time_sequence: times must be (T,), got %s" % (tuple(times.shape),))
    T = int(times.shape[0])
    cams = list(viewpoint_camera) if isinstance(viewpoint_camera, (list, tuple)) else None
    if cams is not None and len(cams) != T:
        raise ValueError("render_time_sequence: %d cameras for %d times" % (len(cams), T))
    chunk = max(1, int(chunk))
    iso = bool(getattr(pc, "use_isotropic_gs", False))
    for c0 in range(0, T, chunk):
        seq = warp.deform_sequence(x, times[c0:c0 + chunk], pc.feature, pc.motion_mask)
        if iso:
            seq["d_rotation"], seq["d_scaling"] = torch.zeros_like(seq["d_rotation"]), torch.zeros_like(seq["d_scaling"])
        at = lambda k, f: None if seq[k] is None else seq[k][f]  # noqa: E731
        for f in range(seq["d_xyz"].shape[0]):
            cam = viewpoint_camera if cams is None else cams[c0 + f]
            with torch.no_grad():
                pkg = render(cam, pc, pipe, bg_color, seq["d_xyz"][f], seq["d_rotation"][f], seq["d_scaling"][f],
                             d_opacity=at("d_opacity", f), d_color=at("d_color", f), d_rot_as_res=warp.d_rot_as_res)
            yield pkg, seq["d_nodes"][f]
