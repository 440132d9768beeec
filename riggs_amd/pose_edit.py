"""Editing the pose of a trained rig by hand: the editor's joint drag, and inverse kinematics on the device.

The first four functions mirror the reference editor's edit step (``interactive_GUI.py``): ``callback_keypoint_drag`` :1268-1329
turns ONE picked joint about the view axis (``update_edited_skeleton_pose`` :324-344, ``update_skeleton_pose_by_rotation``
:296-321) and the edit is composed onto the pose of the frame (:397-399, :440-442).  The reference does this on the host, with
NumPy, scipy and two read-backs per mouse event; here it is torch ops that never read back (CPU tensors work as well), so
``viewer.pick_joint``'s device scalar can be handed on as it is.

``solve_ik`` is what the reference lacks: drag up to 8 end effectors and let the chain follow — damped least squares (Wampler
1986) with Buss & Kim's clamped target step on the rig's own kinematics, every iteration inside ONE launch of csrc/ik.hip
(include/riggs_hip.h: riggs_ik_solve; tests/ik_ref.py is the NumPy restatement).  ``fit_pose`` gives EVERY joint a target
(a reference skeleton, a frame of a clip of joint positions): Levenberg-Marquardt with matrix-free preconditioned conjugate
gradients in ONE launch of csrc/fit.hip (riggs_fit_pose; tests/fit_ref.py).  ``fit_bones`` gives every BONE a target direction,
which a skeleton of other proportions can supply (csrc/bones.hip, riggs_fit_bones; tests/bones_ref.py); ``bone_directions`` takes
the directions from another skeleton's joints and ``retarget`` turns a clip of them into a pose track.  ``fit_rays`` holds every
joint to LINES in space and / or a point (csrc/rays.hip, riggs_fit_rays; tests/rays_ref.py): ``camera_rays`` turns 2-D keypoints
into such lines and ``fit_keypoints`` poses the rig from the keypoints of calibrated cameras, or from the editor's cursor.
Inference only."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .dual_quaternion import quaternion_multiply

MAX_HANDLES, MAX_JOINTS = L.CONSTANTS["RIGGS_IK_MAX_HANDLES"], 256
MAX_RAYS = L.CONSTANTS["RIGGS_RAYS_MAX"]


# --------------------------------------------------------------------------- the reference's edit step
def _matrix(camera, name, like=None):
    m = getattr(camera, name)
    return m if like is None else m.to(like.device)


def view_axis(camera):
    """:337-339 — ``([0, 0, 1, 1] @ inverse(full_proj_transform))[:3]``, normalised: the axis the editor turns a joint about."""
    m = _matrix(camera, "full_proj_transform").float()
    d = (torch.tensor([[0.0, 0.0, 1.0, 1.0]], dtype=m.dtype, device=m.device) @ torch.inverse(m))[0, :3]
    return d / d.norm()


def _project_editor(camera, points):
    """The editor's projection (:1314-1316; x is scaled by ``image_height`` and y by ``image_width``, as the reference writes it):
    ``viewer._project(want_uv=True)`` on the device, the same rule in torch ops for CPU tensors."""
    if points.is_cuda:
        from . import viewer
        return viewer._project(camera, points, viewer.LAYOUT_SQUARES, want_table=False, want_uv=True)[1]
    m = _matrix(camera, "full_proj_transform", points).float()
    hom = torch.cat([points, torch.ones_like(points[:, :1])], dim=1) @ m
    return (hom[:, :2] / hom[:, 3:] + 1) / 2 * torch.tensor([float(camera.image_height), float(camera.image_width)], device=points.device)


@torch.no_grad()
def joint_drag(camera, d_nodes, parents, joint, mouse_xy, mouse_delta=None, cam_rot=None):
    """:1296-1325 — what a drag of the picked ``joint`` to the mouse position means: ``(angle, translation)``, a 0-d and a (3,)
    tensor on ``d_nodes``'s device.

    The root joint (index 0; ``parents[0] < 0`` in the reference): angle 0 and ``0.001 * cam_rot @ [dx, -dy, 0]`` with
    ``mouse_delta = (dx, dy)`` and ``cam_rot`` the (3, 3) camera rotation (:1302-1305).  Any other joint: translation 0 and the
    signed angle in the image between (parent -> joint) and (parent -> mouse), its sign that of the 2-D cross product
    (:1307-1325); ``mouse_xy`` is truncated to integers as the reference does (:1300).  ``joint`` may be a Python integer or a
    0-d integer tensor (``viewer.pick_joint``'s); both cases are evaluated and selected on the device, nothing is read back.
    One deviation: the cosine is clamped to [-1, 1] before ``acos`` — rounding can take the reference's just past 1, which gives NaN."""
    d_nodes = d_nodes.detach().float()
    dev = d_nodes.device
    joint = torch.as_tensor(joint, device=dev).long().reshape(())
    parents = torch.as_tensor(parents, device=dev).long()
    parent = parents[joint].clamp(min=0)
    uv = _project_editor(camera, d_nodes.contiguous())
    mouse = torch.tensor([float(int(mouse_xy[0])), float(int(mouse_xy[1]))], device=dev)
    vec_a = uv[joint] - uv[parent]
    vec_b = mouse - uv[parent]
    cos = (vec_a * vec_b).sum() / (vec_a.norm() * vec_b.norm() + 1e-16)
    angle = torch.acos(cos.clamp(-1.0, 1.0))
    cross = vec_a[0] * vec_b[1] - vec_a[1] * vec_b[0]
    angle = torch.where(cross < 0, -angle, angle)
    is_root = joint == 0
    trans = torch.zeros(3, device=dev)
    if mouse_delta is not None:
        rot = torch.eye(3, device=dev) if cam_rot is None else torch.as_tensor(cam_rot, dtype=torch.float32, device=dev)[:3, :3]
        trans = 0.001 * rot @ torch.tensor([float(mouse_delta[0]), -float(mouse_delta[1]), 0.0], device=dev)
    zero = torch.zeros((), device=dev)
    return torch.where(is_root, zero, angle), torch.where(is_root, trans, torch.zeros_like(trans))


def rotvec_to_quaternion(rotvec):
    """``scipy.spatial.transform.Rotation.from_rotvec(v).as_quat()`` reordered to wxyz (:298-300, :320), in torch ops: the unit
    quaternion (cos(t/2), sin(t/2) v / t), t = |v|, with scipy's series sin(t/2)/t = 1/2 - t^2/48 + t^4/3840 below t = 1e-3."""
    t = rotvec.norm(dim=-1, keepdim=True)
    t2 = t * t
    small = t <= 1e-3
    k = torch.where(small, 0.5 - t2 / 48 + t2 * t2 / 3840, torch.sin(t / 2) / torch.where(small, torch.ones_like(t), t))
    return torch.cat([torch.cos(t / 2), k * rotvec], dim=-1)


@torch.no_grad()
def rotate_joint(edit, joint, axis, angle, translation=None, num_joints=None):
    """:296-321 — the edit ``{'local_rotation': (J, 4), 'global_trans': (1, 3)}`` with row ``joint`` OVERWRITTEN (not composed) by
    the wxyz quaternion of the rotation vector ``axis * angle`` and ``global_trans`` overwritten by ``translation`` (zeros if
    None).  ``edit = None`` creates one of ``num_joints`` identity rows first, on ``axis``'s device (:313-317: the reference sizes
    it by its skeleton); an existing edit is changed in place and returned.  ``joint`` and ``angle`` may be device scalars."""
    if edit is None:
        if num_joints is None:
            raise ValueError("rotate_joint: a new edit needs num_joints")
        axis = torch.as_tensor(axis, dtype=torch.float32)
        q = torch.zeros(int(num_joints), 4, dtype=torch.float32, device=axis.device)
        q[:, 0] = 1
        edit = {"local_rotation": q, "global_trans": torch.zeros(1, 3, device=axis.device)}
    q = edit["local_rotation"]
    axis = torch.as_tensor(axis, dtype=q.dtype, device=q.device)
    angle = torch.as_tensor(angle, dtype=q.dtype, device=q.device)
    joint = torch.as_tensor(joint, device=q.device).long().reshape(1)
    q.index_copy_(0, joint, rotvec_to_quaternion(axis * angle)[None])
    if translation is None:
        edit["global_trans"] = torch.zeros(1, 3, dtype=q.dtype, device=q.device)
    else:
        edit["global_trans"] = torch.as_tensor(translation, dtype=q.dtype, device=q.device).reshape(1, 3)
    return edit


def apply_edit(node_attrs, edit):
    """:397-399 — the pose of the frame with the edit on it: ``local_rotation = quaternion_multiply(edit, pose)`` (the Hamilton
    product, real part made non-negative as the reference's function does), ``global_trans`` summed.  A new dict; other keys are kept."""
    out = dict(node_attrs)
    if edit is not None:
        out["local_rotation"] = quaternion_multiply(edit["local_rotation"], node_attrs["local_rotation"])
        out["global_trans"] = node_attrs["global_trans"] + edit["global_trans"]
    return out


# --------------------------------------------------------------------------- inverse kinematics
def rig_extent(joints):
    """The largest axis range of the rest joints as a (1,) device tensor; 1 where it is 0 (one joint, or all in one place)."""
    e = (joints.max(dim=0).values - joints.min(dim=0).values).max().reshape(1)
    return torch.where(e > 0, e, torch.ones_like(e))


def _rig(skeleton):
    """(joints (J, 3) float32, parents (J,) int32 with 0 at the root) on the device."""
    if isinstance(skeleton, (tuple, list)):
        joints, parents = skeleton
        joints = L.require_cuda_f32("joints", joints.detach(), (None, 3))
        if not torch.is_tensor(parents) or not parents.is_cuda:  # host data: checked here (a device tensor is clamped by the kernel)
            p = np.asarray(parents.cpu() if torch.is_tensor(parents) else parents).astype(np.int64).reshape(-1).copy()
            if p.shape[0] != joints.shape[0]:
                raise L.RiggsHipError("parents has %d entries for %d joints" % (p.shape[0], joints.shape[0]))
            p[0] = 0
            if (p[1:] >= np.arange(1, p.shape[0])).any() or (p < 0).any():
                raise L.RiggsHipError("0 <= parents[i] < i is required (skeleton_warp.py:257-263)")
            parents = torch.from_numpy(p)
        parents = parents.to(joints.device, torch.int32).contiguous()
        if parents.numel() != joints.shape[0]:
            raise L.RiggsHipError("parents has %d entries for %d joints" % (parents.numel(), joints.shape[0]))
        return joints, parents
    joints = skeleton._joints()
    return L.require_cuda_f32("joints", joints, (None, 3)), skeleton._parents_dev(joints.device)


def _problem(name, skeleton, pose, locked, iterations, damping, max_step):
    """What ``solve_ik`` and ``fit_pose`` share in front of their own arguments: the rig, the pose, ``locked``, and the host
    values ``damping`` / ``max_step`` with the ``relative`` mask of their defaults (0.05 and 0.5 times the rig's extent).
    -> (joints, parents, J, q, gt (n, 3), locked, damping, max_step, relative)."""
    joints, parents = _rig(skeleton)
    dev, J = joints.device, int(joints.shape[0])
    if not 1 <= J <= MAX_JOINTS:
        raise L.RiggsHipError("%s: %d joints, 1 to %d are supported" % (name, J, MAX_JOINTS))
    q = L.require_cuda_f32("local_rotation", pose["local_rotation"].detach())
    if q.dim() not in (2, 3) or tuple(q.shape[-2:]) != (J, 4):
        raise L.RiggsHipError("local_rotation has shape %s, expected (%d, 4) or (B, %d, 4)" % (tuple(q.shape), J, J))
    gt = L.require_cuda_f32("global_trans", pose["global_trans"].detach())
    if locked is not None:
        locked = torch.as_tensor(locked).to(dev)
        if tuple(locked.shape) != (J,):
            raise L.RiggsHipError("locked has shape %s, expected (%d,)" % (tuple(locked.shape), J))
        locked = (locked != 0).to(torch.uint8).contiguous()
    if int(iterations) < 0:
        raise L.RiggsHipError("%s: iterations >= 0" % name)
    relative = 0
    if damping is None:
        damping, relative = 0.05, relative | 1
    elif not float(damping) > 0:
        raise L.RiggsHipError("%s: damping must be > 0, got %r" % (name, damping))
    if max_step is None:
        max_step, relative = 0.5, relative | 2
    elif not float(max_step) >= 0:
        raise L.RiggsHipError("%s: max_step must be >= 0, got %r" % (name, max_step))
    return joints, parents, J, q, gt.reshape(-1, 3), locked, float(damping), float(max_step), relative


def _batch(name, q, gt, per_problem):
    """The batch: what has a leading dimension names B, the rest is shared.  ``per_problem``: (tensor or None, its number of
    dimensions when batched) of the caller's own arguments.  -> (B, batched, full) with ``full(t, tail)`` the (B, *tail) contiguous
    form of ``t``: a view where the tensor already is one, so a graph replay sees in-place changes."""
    named = [(q, 3)] + list(per_problem)
    batched = any(t is not None and t.dim() == d for t, d in named) or gt.shape[0] > 1
    sizes = {int(t.shape[0]) for t, d in named + [(gt, 2)] if t is not None and t.dim() == d}
    sizes.discard(1)
    if len(sizes) > 1:
        raise L.RiggsHipError("%s: the arguments name different batch sizes %s" % (name, sorted(sizes)))
    B = sizes.pop() if sizes else 1
    if gt.numel() not in (3, 3 * B):
        raise L.RiggsHipError("global_trans has shape %s, expected (1, 3) or (%d, 3)" % (tuple(gt.shape), B))

    def full(t, tail):
        return t.reshape((-1,) + tail).expand((B,) + tail).contiguous()
    return B, batched, full


def _solution(batched, q_out, gt_out, d_nodes, residual):
    if batched:
        return {"local_rotation": q_out, "global_trans": gt_out, "d_nodes": d_nodes, "residual": residual}
    return {"local_rotation": q_out[0], "global_trans": gt_out, "d_nodes": d_nodes[0], "residual": residual[0]}


@torch.no_grad()
def solve_ik(skeleton, pose, handles, targets, weights=None, locked=None, iterations=16, damping=None, max_step=None,
             solve_translation=False):
    """Turn the joints of ``pose`` so that the ``handles`` joints reach ``targets``; the chain follows.

    ``skeleton``: a ``SkeletonWarp`` or ``(joints (J, 3), parents (J,))``, 1 <= J <= 256.  ``pose``: the dict ``deform_by_pose`` /
    ``get_pose_info`` use — ``local_rotation`` (J, 4) or (B, J, 4), un-normalised wxyz; ``global_trans`` (1, 3) or (B, 3).
    ``handles``: (E,) or (B, E) joint indices, 1 <= E <= 8 (targets for more joints, up to every one: ``fit_pose``); ``targets``
    (..., E, 3); ``weights`` (..., E), a weight <= 0 switches
    its handle off (so the number of live handles changes without a new shape); ``locked`` (J,) bool: joints that keep their
    rotation.  Unbatched arguments are shared by the B problems.  ``damping`` (> 0) and ``max_step`` default to 0.05 and 0.5 times
    ``rig_extent(joints)``, which stays on the device.  ``solve_translation``: ``global_trans`` is solved for as well.
    Where a target may be out of reach, give a ``damping`` of about ``max_step``: with the small default the stretched chain
    swings from iteration to iteration instead of settling (the method's behaviour, in float64 as well).

    Returns ``{'local_rotation', 'global_trans', 'd_nodes', 'residual'}``: the pose (the input's shapes; it feeds
    ``deform_by_pose``, ``deform_sequence`` and ``run_interpolation`` unchanged), the posed skeleton (..., J, 3) for
    ``skeleton_overlay`` and ``|target - posed handle|`` (..., E).  The iteration is stated in include/riggs_hip.h.

    One launch, allocations through torch only, nothing read back: the call can be captured in a ``torch.cuda.graph`` and
    replayed after ``targets`` / ``handles`` / ``weights`` (device tensors) were changed in place.  Handle indices given on the
    host (a list, an array, a CPU tensor) are checked here; on the device they are not read: the kernel switches off a handle
    outside [0, J) and reports NaN as its residual."""
    joints, parents, J, q, gt, locked, damping, max_step, relative = _problem("solve_ik", skeleton, pose, locked, iterations, damping, max_step)
    dev = joints.device
    if torch.is_tensor(handles) and handles.is_cuda:
        h = handles
    else:
        h_host = np.asarray(handles.cpu() if torch.is_tensor(handles) else handles)
        if h_host.size and (not np.issubdtype(h_host.dtype, np.integer) or h_host.min() < 0 or h_host.max() >= J):
            raise L.RiggsHipError("solve_ik: a handle is no joint index in [0, %d)" % J)
        h = torch.from_numpy(h_host.astype(np.int32)).to(dev)
    if h.dim() not in (1, 2) or not 1 <= h.shape[-1] <= MAX_HANDLES:
        raise L.RiggsHipError("solve_ik: handles has shape %s, expected (E,) or (B, E) with 1 <= E <= %d" % (tuple(h.shape), MAX_HANDLES))
    E = int(h.shape[-1])
    targets = L.require_cuda_f32("targets", targets.detach())
    if targets.dim() not in (2, 3) or tuple(targets.shape[-2:]) != (E, 3):
        raise L.RiggsHipError("targets has shape %s, expected (..., %d, 3)" % (tuple(targets.shape), E))
    if weights is not None:
        weights = L.require_cuda_f32("weights", weights.detach())
        if weights.dim() not in (1, 2) or weights.shape[-1] != E:
            raise L.RiggsHipError("weights has shape %s, expected (..., %d)" % (tuple(weights.shape), E))
    extent = rig_extent(joints) if relative else None
    B, batched, full = _batch("solve_ik", q, gt, [(h, 2), (targets, 3), (weights, 2)])
    qb, gtb, hb, tb = full(q, (J, 4)), full(gt, (3,)), full(h.to(torch.int32), (E,)), full(targets, (E, 3))
    wb = None if weights is None else full(weights, (E,))
    f32 = dict(dtype=torch.float32, device=dev)
    q_out, gt_out = torch.empty(B, J, 4, **f32), torch.empty(B, 3, **f32)
    d_nodes, residual = torch.empty(B, J, 3, **f32), torch.empty(B, E, **f32)
    with torch.cuda.device(dev):
        L.check(L.lib().riggs_ik_solve(B, J, E, joints.data_ptr(), parents.data_ptr(), qb.data_ptr(), gtb.data_ptr(), hb.data_ptr(),
                                       tb.data_ptr(), L.ptr(wb), L.ptr(locked), int(iterations), damping, max_step,
                                       L.ptr(extent), relative, int(bool(solve_translation)), q_out.data_ptr(), gt_out.data_ptr(),
                                       d_nodes.data_ptr(), residual.data_ptr(), L.stream_ptr()), "riggs_ik_solve")
    return _solution(batched, q_out, gt_out, d_nodes, residual)


@torch.no_grad()
def fit_pose(skeleton, pose, targets, weights=None, locked=None, iterations=32, cg_steps=8, damping=None, max_step=None,
             solve_translation=False):
    """Turn the joints of ``pose`` so that EVERY joint reaches its own target: matching the rig to a reference skeleton, turning
    a clip of joint positions into a pose track, re-posing a rig whose rest joints were extracted anew.

    ``skeleton``, ``pose``, ``locked``, ``damping``, ``max_step``, ``solve_translation`` and the batching are ``solve_ik``'s.
    ``targets``: (J, 3) or (B, J, 3), one per joint; ``weights`` (J,) or (B, J), all 1 by default: a weight <= 0 means that the
    joint has no target, and its entry of ``targets`` is never read (a NaN there changes no bit of the result).
    ``cg_steps`` (>= 1): conjugate-gradient steps per iteration.  More steps than joints gain nothing, and they make the twist
    about a bone, which no position observes, depend on the order of the sums: rotations then differ by 1e-2 between
    implementations while the positions agree.  Keep ``cg_steps <= J``.

    The method: Levenberg-Marquardt on the rig's kinematics with the clamped target step, the damped normal equations solved
    matrix-free by Jacobi-preconditioned conjugate gradients, where the Jacobian of the tree and its transpose are two sweeps
    over its levels (include/riggs_hip.h states the iteration, tests/fit_ref.py restates it in NumPy).

    Returns ``{'local_rotation', 'global_trans', 'd_nodes', 'residual'}`` as ``solve_ik`` does, with ``residual`` (..., J):
    ``|target - posed joint|`` where the weight is > 0, and 0 elsewhere.  A (B, J, 4) result is a track for ``deform_sequence``.

    One launch of csrc/fit.hip, allocations through torch only, nothing read back: the call can be captured in a
    ``torch.cuda.graph`` (with ``deform_by_pose`` behind it) and replayed after ``targets`` / ``weights`` changed in place."""
    if int(cg_steps) < 1:
        raise L.RiggsHipError("fit_pose: cg_steps must be >= 1, got %r" % (cg_steps,))
    joints, parents, J, q, gt, locked, damping, max_step, relative = _problem("fit_pose", skeleton, pose, locked, iterations, damping, max_step)
    dev = joints.device
    targets = L.require_cuda_f32("targets", targets.detach())
    if targets.dim() not in (2, 3) or tuple(targets.shape[-2:]) != (J, 3):
        raise L.RiggsHipError("targets has shape %s, expected (%d, 3) or (B, %d, 3)" % (tuple(targets.shape), J, J))
    if weights is not None:
        weights = L.require_cuda_f32("weights", weights.detach())
        if weights.dim() not in (1, 2) or weights.shape[-1] != J:
            raise L.RiggsHipError("weights has shape %s, expected (%d,) or (B, %d)" % (tuple(weights.shape), J, J))
    extent = rig_extent(joints)  # (always: the translation unknown is scaled by it)
    B, batched, full = _batch("fit_pose", q, gt, [(targets, 3), (weights, 2)])
    qb, gtb, tb = full(q, (J, 4)), full(gt, (3,)), full(targets, (J, 3))
    wb = None if weights is None else full(weights, (J,))
    f32 = dict(dtype=torch.float32, device=dev)
    q_out, gt_out = torch.empty(B, J, 4, **f32), torch.empty(B, 3, **f32)
    d_nodes, residual = torch.empty(B, J, 3, **f32), torch.empty(B, J, **f32)
    with torch.cuda.device(dev):
        L.check(L.lib().riggs_fit_pose(B, J, joints.data_ptr(), parents.data_ptr(), qb.data_ptr(), gtb.data_ptr(), tb.data_ptr(),
                                       L.ptr(wb), L.ptr(locked), int(iterations), int(cg_steps), damping, max_step,
                                       extent.data_ptr(), relative, int(bool(solve_translation)), q_out.data_ptr(),
                                       gt_out.data_ptr(), d_nodes.data_ptr(), residual.data_ptr(), L.stream_ptr()), "riggs_fit_pose")
    return _solution(batched, q_out, gt_out, d_nodes, residual)


# --------------------------------------------------------------------------- bone directions: skeletons of other proportions
@torch.no_grad()
def fit_bones(skeleton, pose, directions, weights=None, locked=None, iterations=32, cg_steps=8, damping=0.05, max_step=0.5):
    """Turn the joints of ``pose`` so that every BONE (joint h >= 1 and its parent) points along its own target direction.  A
    direction does not depend on the length of the bone it was taken from, so the targets may come from a skeleton of other
    proportions (a motion-capture clip, another rig's ``d_nodes``, a rest skeleton extracted anew), where position targets that
    no pose can reach make ``fit_pose`` bend every joint into a compromise.

    ``skeleton``, ``pose``, ``locked``, ``cg_steps`` and the batching are ``fit_pose``'s.  ``directions``: (J, 3) or (B, J, 3), a
    vector of any length along the target of bone h in row h; row 0 is ignored (the root has no bone).  ``weights`` (J,) or (B, J),
    all 1 by default.  A bone has no target where its weight is <= 0, where its rest length is 0 or where its target vector has
    length 0 (or is NaN); without weight or rest length the row of ``directions`` is never read.  ``damping`` (> 0) and
    ``max_step`` (>= 0) are absolute: they act on unit vectors, whatever the rig's size.  No translation is solved for:
    ``global_trans`` is returned as it came (``retarget`` sets it from the source's root).

    The method is ``fit_pose``'s on the unit bone vectors; because the rig is rigid a bone only turns, by the sum of the rotation
    unknowns along its path, so the Jacobian and its transpose are sweeps of 3 values (include/riggs_hip.h states the iteration,
    tests/bones_ref.py restates it in NumPy).  The twist about a bone is not observed and stays where it was.

    Returns ``{'local_rotation', 'global_trans', 'd_nodes', 'residual'}`` as ``fit_pose`` does, with ``residual`` (..., J) the
    chord ``|t - d|`` between the target and the posed unit direction (in [0, 2]; 0 where the bone has no target).

    One launch of csrc/bones.hip, allocations through torch only, nothing read back: the call can be captured in a
    ``torch.cuda.graph`` and replayed after ``directions`` / ``weights`` changed in place."""
    if int(cg_steps) < 1:
        raise L.RiggsHipError("fit_bones: cg_steps must be >= 1, got %r" % (cg_steps,))
    damping, max_step = 0.05 if damping is None else damping, 0.5 if max_step is None else max_step
    joints, parents, J, q, gt, locked, damping, max_step, _ = _problem("fit_bones", skeleton, pose, locked, iterations, damping, max_step)
    dev = joints.device
    directions = L.require_cuda_f32("directions", directions.detach())
    if directions.dim() not in (2, 3) or tuple(directions.shape[-2:]) != (J, 3):
        raise L.RiggsHipError("directions has shape %s, expected (%d, 3) or (B, %d, 3)" % (tuple(directions.shape), J, J))
    if weights is not None:
        weights = L.require_cuda_f32("weights", weights.detach())
        if weights.dim() not in (1, 2) or weights.shape[-1] != J:
            raise L.RiggsHipError("weights has shape %s, expected (%d,) or (B, %d)" % (tuple(weights.shape), J, J))
    B, batched, full = _batch("fit_bones", q, gt, [(directions, 3), (weights, 2)])
    qb, gtb, db = full(q, (J, 4)), full(gt, (3,)), full(directions, (J, 3))
    wb = None if weights is None else full(weights, (J,))
    f32 = dict(dtype=torch.float32, device=dev)
    q_out, gt_out = torch.empty(B, J, 4, **f32), torch.empty(B, 3, **f32)
    d_nodes, residual = torch.empty(B, J, 3, **f32), torch.empty(B, J, **f32)
    with torch.cuda.device(dev):
        L.check(L.lib().riggs_fit_bones(B, J, joints.data_ptr(), parents.data_ptr(), qb.data_ptr(), gtb.data_ptr(), db.data_ptr(),
                                        L.ptr(wb), L.ptr(locked), int(iterations), int(cg_steps), damping, max_step,
                                        q_out.data_ptr(), gt_out.data_ptr(), d_nodes.data_ptr(), residual.data_ptr(),
                                        L.stream_ptr()), "riggs_fit_bones")
    return _solution(batched, q_out, gt_out, d_nodes, residual)


def _virtual_parents(parents, dev):
    """(J,) long on ``dev`` with the kernels' rule: 0 at the root, a value outside [0, i) clamped into it."""
    p = torch.as_tensor(parents).to(dev).long().reshape(-1)
    below = (torch.arange(p.numel(), device=dev) - 1).clamp(min=0)
    return torch.minimum(p.clamp(min=0), below)


@torch.no_grad()
def bone_directions(joints, parents, joint_map=None):
    """The bones of another skeleton as ``fit_bones`` takes them: ``(directions (..., J, 3), weights (..., J))``.

    ``joints``: (Js, 3) or (T, Js, 3), the SOURCE skeleton's joints (one frame or a clip); ``parents`` (J,): the RIG's parents;
    ``joint_map`` (J,) integers: the source joint that stands for rig joint h, -1 for none (an index outside [0, Js) counts as
    none).  Default: the identity, which needs Js == J.  ``directions[h] = src[map[h]] - src[map[vp(h)]]``, and the weight is 1
    where h >= 1 and both ends are mapped, else 0 (with a zero direction).  Torch ops on ``joints``'s device, nothing read back."""
    src = joints.detach().float()
    if src.dim() not in (2, 3) or src.shape[-1] != 3:
        raise L.RiggsHipError("bone_directions: joints has shape %s, expected (Js, 3) or (T, Js, 3)" % (tuple(src.shape),))
    dev, Js = src.device, int(src.shape[-2])
    vp = _virtual_parents(parents, dev)
    J = int(vp.numel())
    idx = torch.arange(J, device=dev)
    if joint_map is None:
        if Js != J:
            raise L.RiggsHipError("bone_directions: %d source joints for %d rig joints need a joint_map" % (Js, J))
        m = idx
    else:
        m = torch.as_tensor(joint_map).to(dev).long().reshape(-1)
        if m.numel() != J:
            raise L.RiggsHipError("bone_directions: joint_map has %d entries for %d rig joints" % (m.numel(), J))
    if Js < 1:
        raise L.RiggsHipError("bone_directions: the source has no joints")
    mapped = (m >= 0) & (m < Js)
    mc = m.clamp(0, Js - 1)
    ok = mapped & mapped[vp] & (idx >= 1)
    d = src.index_select(-2, mc) - src.index_select(-2, mc[vp])
    d = torch.where(ok[:, None], d, torch.zeros_like(d))
    return d, ok.to(src.dtype).expand(d.shape[:-1]).contiguous()


@torch.no_grad()
def root_follow(joints, parents, source_joints, joint_map=None, root_scale=None, global_trans=None, weights=None):
    """``retarget``'s root motion: ``k * src[map[0]]_t - joints[0]`` per frame, (T, 3).  ``k = root_scale`` or, if that is None,
    the summed rest lengths of the rig's live bones (mapped at both ends, ``weights`` > 0 where given, rest and source length > 0)
    over the same bones' lengths in the source's first frame; 1 where no bone is live.  A root that is not mapped gives
    ``global_trans`` (zeros if None) instead.  Torch ops on the device of ``joints``, nothing read back."""
    joints = joints.detach().float()
    dev, J = joints.device, int(joints.shape[0])
    src = source_joints.detach().float().to(dev)
    Js = int(src.shape[-2])
    clip = src.reshape(-1, Js, 3)
    m0 = torch.zeros((), dtype=torch.long, device=dev) if joint_map is None else torch.as_tensor(joint_map).to(dev).long().reshape(-1)[0]
    if root_scale is None:
        rest = (joints - joints[_virtual_parents(parents, dev)]).norm(dim=-1)
        d, w = bone_directions(clip[0], parents, joint_map)
        if weights is not None:
            w = w * weights.reshape(-1, J)[0]
        length = d.norm(dim=-1)
        live = (w > 0) & (rest > 0) & (length > 0)
        zero = torch.zeros_like(rest)
        num, den = torch.where(live, rest, zero).sum(), torch.where(live, length, zero).sum()
        k = torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.ones_like(den))
    else:
        k = torch.as_tensor(root_scale, dtype=torch.float32, device=dev)
    follow = k * clip.index_select(1, m0.clamp(0, Js - 1).reshape(1))[:, 0] - joints[0]
    keep = torch.zeros_like(follow) if global_trans is None else global_trans.reshape(-1, 3).expand(follow.shape[0], 3)
    return torch.where((m0 >= 0) & (m0 < Js), follow, keep).contiguous()


@torch.no_grad()
def retarget(skeleton, pose, source_joints, joint_map=None, root_motion="none", root_scale=None, **fit_bones_kw):
    """A clip of another skeleton's joints -> a pose track of the rig: the T frames are one batch of T independent problems of
    ``fit_bones`` on the clip's bone directions (``bone_directions``), whatever the source's proportions.

    ``source_joints``: (T, Js, 3) (or (Js, 3): one frame); ``joint_map`` as in ``bone_directions``; ``pose``: the starting pose,
    (J, 4) shared by the frames or (T, J, 4).  ``root_motion``: "none" keeps ``pose['global_trans']``; "follow" puts the rig's root
    where the source's is, ``global_trans_t = k * src[map[0]]_t - joints[0]`` (a root that is not mapped keeps the pose's
    translation), with ``k = root_scale`` or, if that is None, the summed rest lengths of the rig's live bones over the same
    bones' lengths in the source's FIRST frame (1 where there is none), computed on the device.  Further keywords go to
    ``fit_bones``; its ``weights`` multiply the mapping's.

    Returns ``fit_bones``'s dict: a (T, J, 4) / (T, 3) track that feeds ``deform_sequence``, ``render_sequence`` and
    ``run_interpolation`` unchanged, and ``d_nodes`` (T, J, 3) for ``skeleton_overlay``.  Frames are solved independently: nothing
    smooths across them."""
    if root_motion not in ("none", "follow"):
        raise L.RiggsHipError("retarget: root_motion must be 'none' or 'follow', got %r" % (root_motion,))
    joints, parents = _rig(skeleton)
    src = L.require_cuda_f32("source_joints", source_joints.detach())
    directions, weights = bone_directions(src, parents, joint_map)
    extra = fit_bones_kw.pop("weights", None)
    if extra is not None:
        weights = weights * L.require_cuda_f32("weights", extra.detach())
    gt = pose["global_trans"]
    if root_motion == "follow":
        gt = root_follow(joints, parents, src, joint_map, root_scale, L.require_cuda_f32("global_trans", gt.detach()), weights)
    return fit_bones((joints, parents), {"local_rotation": pose["local_rotation"], "global_trans": gt}, directions, weights=weights,
                     **fit_bones_kw)


# --------------------------------------------------------------------------- lines and points: 2-D keypoints, the editor's cursor
@torch.no_grad()
def fit_rays(skeleton, pose, origins, directions, weights=None, pins=None, pin_weights=None, locked=None, iterations=32, cg_steps=8,
             damping=None, max_step=None, solve_translation=False):
    """Turn the joints of ``pose`` so that every joint comes to lie on its LINES (the ray through a camera centre and a keypoint,
    the editor's cursor) and / or at its PIN (a point: ``fit_pose``'s target).  Rays and pins mix freely; two or more rays of a
    joint from different origins triangulate it within the solve.

    ``skeleton``, ``pose``, ``locked``, ``iterations``, ``cg_steps``, ``damping``, ``max_step``, ``solve_translation``, the
    batching and the defaults are ``fit_pose``'s.  ``origins`` / ``directions``: (J, K, 3) or (B, J, K, 3), 1 <= K <= 8 lines per
    joint, each through ``origins`` along ``directions`` (any length); ``origins`` may also be (K, 3), shared by all joints and
    problems (K cameras).  ``weights`` (J, K) or (B, J, K), default 1.  ``pins`` (J, 3) or (B, J, 3) with ``pin_weights`` (J,) or
    (B, J), default 1 where ``pins`` is given.  ``origins = directions = None`` with pins is ``fit_pose``'s problem (K = 0).
    A ray counts where its weight is > 0 and its direction is non-zero and finite, a pin where its weight is > 0; a weight <= 0
    or NaN switches off, and what is switched off is never used: a NaN there changes no bit of the result.  Per-frame cameras of a
    clip are this function's job (``fit_keypoints`` shares its cameras among the batch): build (B, J, K, 3) rays with
    ``camera_rays`` per frame.

    The method is ``fit_pose``'s with a symmetric 3 x 3 metric per joint, ``wp I + sum_k w_k (I - d_k d_k^T)``, in place of its
    scalar weight (include/riggs_hip.h states the iteration, tests/rays_ref.py restates it in NumPy).  Limits: a line extends
    behind its origin (a line, not a half-line); what is minimised is the distance to the line — the reprojection error times
    depth / focal length — not the pixel error; with ONE ray per joint the position along the ray is held only by the damping and
    the starting pose; two-camera problems can have genuine local minima (a near-antipodal pair on a chain); at 64 and more
    joints 32 iterations have not converged: raise ``iterations``.  Joint limits, orientation targets, smoothing across frames and
    lens distortion are out of scope.

    Returns ``{'local_rotation', 'global_trans', 'd_nodes', 'residual'}`` as ``fit_pose`` does, with ``residual`` (..., J) the
    largest distance of the posed joint to one of its live lines or its pin, in world units; 0 where the joint has none.

    One launch of csrc/rays.hip, allocations through torch only, nothing read back: the call can be captured in a
    ``torch.cuda.graph`` and replayed after the rays, pins and weights changed in place."""
    if int(cg_steps) < 1:
        raise L.RiggsHipError("fit_rays: cg_steps must be >= 1, got %r" % (cg_steps,))
    if (origins is None) != (directions is None):
        raise L.RiggsHipError("fit_rays: origins and directions come together")
    if origins is None and weights is not None:
        raise L.RiggsHipError("fit_rays: weights without rays")
    if pins is None and pin_weights is not None:
        raise L.RiggsHipError("fit_rays: pin_weights without pins")
    if origins is None and pins is None:
        raise L.RiggsHipError("fit_rays: neither rays nor pins")
    K = 0
    if directions is not None:
        if directions.dim() not in (3, 4) or directions.shape[-1] != 3:
            raise L.RiggsHipError("directions has shape %s, expected (J, K, 3) or (B, J, K, 3)" % (tuple(directions.shape),))
        K = int(directions.shape[-2])
        if not 1 <= K <= MAX_RAYS:
            raise L.RiggsHipError("fit_rays: %d rays per joint, 1 to %d are supported" % (K, MAX_RAYS))
        if tuple(origins.shape) != (K, 3) and (origins.dim() not in (3, 4) or tuple(origins.shape[-3:]) != tuple(directions.shape[-3:])):
            raise L.RiggsHipError("origins has shape %s, expected (%d, 3) or (..., %d, %d, 3) as directions"
                                  % (tuple(origins.shape), K, directions.shape[-3], K))
        if weights is not None and (weights.dim() not in (2, 3) or tuple(weights.shape[-2:]) != tuple(directions.shape[-3:-1])):
            raise L.RiggsHipError("weights has shape %s, expected (..., %d, %d)" % (tuple(weights.shape), directions.shape[-3], K))
    if pins is not None:
        if pins.dim() not in (2, 3) or pins.shape[-1] != 3:
            raise L.RiggsHipError("pins has shape %s, expected (J, 3) or (B, J, 3)" % (tuple(pins.shape),))
        if pin_weights is not None and (pin_weights.dim() not in (1, 2) or pin_weights.shape[-1] != pins.shape[-2]):
            raise L.RiggsHipError("pin_weights has shape %s, expected (..., %d)" % (tuple(pin_weights.shape), pins.shape[-2]))
    joints, parents, J, q, gt, locked, damping, max_step, relative = _problem("fit_rays", skeleton, pose, locked, iterations, damping, max_step)
    dev = joints.device
    f32 = dict(dtype=torch.float32, device=dev)
    if K:
        directions = L.require_cuda_f32("directions", directions.detach())
        origins = L.require_cuda_f32("origins", origins.detach())
        weights = L.require_cuda_f32("weights", None if weights is None else weights.detach())
        if directions.shape[-3] != J:
            raise L.RiggsHipError("directions has shape %s, expected (%d, K, 3) or (B, %d, K, 3)" % (tuple(directions.shape), J, J))
        if origins.dim() == 2:
            origins = origins.expand(J, K, 3)
    if pins is not None:
        pins = L.require_cuda_f32("pins", pins.detach())
        pin_weights = L.require_cuda_f32("pin_weights", None if pin_weights is None else pin_weights.detach())
        if pins.shape[-2] != J:
            raise L.RiggsHipError("pins has shape %s, expected (%d, 3) or (B, %d, 3)" % (tuple(pins.shape), J, J))
    extent = rig_extent(joints)  # (always: the translation unknown is scaled by it)
    B, batched, full = _batch("fit_rays", q, gt, [(origins, 4), (directions, 4), (weights, 3), (pins, 3), (pin_weights, 2)])
    qb, gtb = full(q, (J, 4)), full(gt, (3,))
    ob = db = wb = pb = pwb = None
    if K:
        ob, db = full(origins, (J, K, 3)), full(directions, (J, K, 3))
        wb = torch.ones(B, J, K, **f32) if weights is None else full(weights, (J, K))
    if pins is not None:
        pb = full(pins, (J, 3))
        pwb = torch.ones(B, J, **f32) if pin_weights is None else full(pin_weights, (J,))
    q_out, gt_out = torch.empty(B, J, 4, **f32), torch.empty(B, 3, **f32)
    d_nodes, residual = torch.empty(B, J, 3, **f32), torch.empty(B, J, **f32)
    with torch.cuda.device(dev):
        L.check(L.lib().riggs_fit_rays(B, J, K, joints.data_ptr(), parents.data_ptr(), qb.data_ptr(), gtb.data_ptr(), L.ptr(ob),
                                       L.ptr(db), L.ptr(wb), L.ptr(pb), L.ptr(pwb), L.ptr(locked), int(iterations), int(cg_steps),
                                       damping, max_step, extent.data_ptr(), relative, int(bool(solve_translation)),
                                       q_out.data_ptr(), gt_out.data_ptr(), d_nodes.data_ptr(), residual.data_ptr(),
                                       L.stream_ptr()), "riggs_fit_rays")
    return _solution(batched, q_out, gt_out, d_nodes, residual)


def _pinhole(camera, like):
    """(fx, fy, cx, cy) of ``loss.camera_intrinsics`` and the view's rotation R (3, 3) and translation t (3,) on ``like``'s device,
    in the reference's row-vector convention: camera-space point = world point @ R + t (csrc/pinhole.h: pinhole_view)."""
    from .loss import camera_intrinsics
    V = camera.world_view_transform.detach().to(device=like.device, dtype=torch.float32)
    return camera_intrinsics(camera), V[:3, :3], V[3, :3]


@torch.no_grad()
def camera_rays(camera, keypoints):
    """The lines of sight of 2-D keypoints: ``(origin (3,), directions (..., 3))`` for ``keypoints`` (..., 2) as (x, y) =
    (column, row) in pixels, as ``fit_rays`` takes them.  The inverse of csrc/pinhole.h's rule (column = fx tx / tz + cx,
    row = fy ty / tz + cy with ``loss.camera_intrinsics(camera)``; t = p @ R + T with ``camera.world_view_transform`` in the
    reference's row-vector convention): direction = ((x - cx) / fx, (y - cy) / fy, 1) @ R^-1, origin = -T @ R^-1, the camera's
    centre.  R^-1 is formed from R's cofactors in torch ops on the keypoints' device (CPU tensors work as well): nothing is read
    back.  No lens distortion."""
    kp = keypoints.detach().float()
    if kp.shape[-1] != 2:
        raise L.RiggsHipError("camera_rays: keypoints has shape %s, expected (..., 2)" % (tuple(kp.shape),))
    (fx, fy, cx, cy), R, t = _pinhole(camera, kp)
    cof = torch.stack([torch.linalg.cross(R[1], R[2]), torch.linalg.cross(R[2], R[0]), torch.linalg.cross(R[0], R[1])], dim=1)
    Rinv = cof / (R[0] * cof[:, 0]).sum()
    # (element-wise, not a matrix product: the same keypoint gives the same bits whatever the shape it arrives in)
    x, y = ((kp[..., 0] - cx) / fx)[..., None], ((kp[..., 1] - cy) / fy)[..., None]
    return -(t[0] * Rinv[0] + t[1] * Rinv[1] + t[2] * Rinv[2]), x * Rinv[0] + y * Rinv[1] + Rinv[2]


@torch.no_grad()
def fit_keypoints(skeleton, pose, cameras, keypoints, weights=None, pins=None, pin_weights=None, **fit_rays_kw):
    """Pose the rig from 2-D keypoints: ``cameras``, a list of 1 <= C <= 8 calibrated cameras shared by the batch, and
    ``keypoints`` (C, J, 2) or (B, C, J, 2) as (x, y) = (column, row) in pixels, one per camera and joint.  ``weights`` (C, J) or
    (B, C, J): the detector's confidences, default 1; a weight <= 0 or NaN means unseen, and an unseen keypoint may hold anything
    (a NaN there changes no bit).  ``pins`` / ``pin_weights`` and further keywords go to ``fit_rays``: the editor's drag is ONE
    call with the cursor as the handle joint's keypoint (weight 0 elsewhere) and pins at the current ``d_nodes`` on the joints
    that stay.  A clip (B = T frames) gives a pose track for ``deform_sequence`` / ``render_sequence``; frames are solved
    independently.  Cameras that change from frame to frame are ``fit_rays``'s job: build its rays with ``camera_rays``.

    The rays come from ``camera_rays``, the solve is ONE launch of ``fit_rays`` (its limits apply: with one camera the depth is
    held only by the damping and the starting pose, and the distance to the ray is minimised, not the pixel error).

    Returns ``fit_rays``'s dict plus ``reprojection`` (..., C, J): the pixel distance between each keypoint and csrc/pinhole.h's
    projection of the returned ``d_nodes``; 0 where the weight is <= 0.  Torch ops on the device, nothing read back: capturable
    (with the cameras' ``world_view_transform`` already on the device: ``camera.to("cuda")``)."""
    cameras = list(cameras)
    kp = L.require_cuda_f32("keypoints", keypoints.detach())
    C = len(cameras)
    if not 1 <= C <= MAX_RAYS:
        raise L.RiggsHipError("fit_keypoints: %d cameras, 1 to %d are supported" % (C, MAX_RAYS))
    if kp.dim() not in (3, 4) or kp.shape[-3] != C or kp.shape[-1] != 2:
        raise L.RiggsHipError("keypoints has shape %s, expected (%d, J, 2) or (B, %d, J, 2)" % (tuple(kp.shape), C, C))
    if weights is not None:
        weights = L.require_cuda_f32("weights", weights.detach())
        if weights.dim() not in (2, 3) or tuple(weights.shape[-2:]) != tuple(kp.shape[-3:-1]):
            raise L.RiggsHipError("weights has shape %s, expected (..., %d, %d)" % (tuple(weights.shape), C, kp.shape[-2]))
    rays = [camera_rays(cam, kp[..., c, :, :]) for c, cam in enumerate(cameras)]
    origins = torch.stack([o for o, _ in rays])            # (C, 3)
    directions = torch.stack([d for _, d in rays], dim=-2)  # (..., J, C, 3)
    out = fit_rays(skeleton, pose, origins, directions, weights=None if weights is None else weights.transpose(-1, -2),
                   pins=pins, pin_weights=pin_weights, **fit_rays_kw)
    posed = out["d_nodes"]
    per_camera = []
    for c, cam in enumerate(cameras):
        (fx, fy, cx, cy), R, t = _pinhole(cam, posed)
        v = posed[..., 0:1] * R[0] + posed[..., 1:2] * R[1] + posed[..., 2:3] * R[2] + t
        dx, dy = fx * v[..., 0] / v[..., 2] + cx - kp[..., c, :, 0], fy * v[..., 1] / v[..., 2] + cy - kp[..., c, :, 1]
        per_camera.append(torch.sqrt(dx * dx + dy * dy))
    reprojection = torch.stack(per_camera, dim=-2)
    if weights is not None:
        reprojection = torch.where(weights > 0, reprojection, torch.zeros_like(reprojection))
    return dict(out, reprojection=reprojection)
