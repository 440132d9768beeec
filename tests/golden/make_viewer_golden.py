"""Golden vectors for the editor's display step (riggs_amd/viewer.py), captured from the REAL RigGS reference on the CPU — run in
the build container only:
    python tests/golden/make_viewer_golden.py
Never imported by a test.  ``utils/other_utils.py`` imports here, so the reference's own ``depth2normal`` is recorded.
``render_rig.py`` and ``interactive_GUI.py`` import once the packages they name at module level but that are absent here
(torchvision, dearpygui, lpips, piq, pytorch_msssim, skimage) are registered as empty stand-ins; their own projection lines then
run unchanged — ``GUI.update_skeleton_edges``, ``update_reference_skeleton``, ``update_trajectory_overlay``,
``update_control_point_overlay`` on a bare stand-in for ``self``, and ``project_nodes_to_2d_withnodes`` — with ``cv2.polylines``,
``cv2.circle`` and ``cv2.rectangle`` replaced by recorders: what is kept is the integer coordinates, radii, thicknesses and
colours they were CALLED with, in call order.  OpenCV itself is absent: nothing it would have drawn is recorded or imitated.

Files (inputs and results only):
  viewer_frames.npz    per depth2normal case the reference's float64 normals and ``dev32``, the largest deviation of its float32 run
                       from them; per frame case ``dev32`` of the reference's lines :521-529, :611-626 (torch ops) in float32
                       against float64 — the tolerances of the GPU test derive from these
  viewer_overlays.npz  the scene (camera matrices, joints, parents, trajectory samples, key point) and the recorded calls
  viewer_jet512.npz    the 512 colours of :147 from matplotlib's "jet"
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _ref_shim as S  # noqa: E402

S.install()


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Absent:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):  # (image_utils.py builds its LPIPS networks at import: ``.net.cuda()``)
        if name.startswith("__"):
            raise AttributeError(name)
        return _Absent()

    def __call__(self, *a, **k):
        return _Absent()


_module("torchvision", utils=_module("torchvision.utils", save_image=lambda *a, **k: None))
_module("dearpygui", dearpygui=_module("dearpygui.dearpygui"))
_module("lpips", LPIPS=_Absent)
_module("piq", ssim=None, LPIPS=_Absent)
_module("pytorch_msssim", ms_ssim=None)
_module("skimage", draw=_module("skimage.draw", line_aa=None))

CALLS = []


def _rec(kind):
    def f(img=None, *a, **k):
        CALLS.append((kind, a, k))
        return img
    return f


cv2 = sys.modules["cv2"]
cv2.polylines, cv2.circle, cv2.rectangle = _rec("polylines"), _rec("circle"), _rec("rectangle")

with S.quiet():
    from utils.other_utils import depth2normal  # noqa: E402
    import interactive_GUI  # noqa: E402
    import render_rig  # noqa: E402

from riggs_amd import synth  # noqa: E402
from tests import viewer_ref as VR  # noqa: E402


def save(name, **kw):
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **kw)
    print("wrote", name, {k: np.asarray(v).shape for k, v in kw.items()})


# --------------------------------------------------------------------------- frames
def reference_frame(out, mode, size, dtype):
    """interactive_GUI.py:521-529 and :611-626 as torch ops on the CPU: (H, W, 3)."""
    out = {k: torch.tensor(v, dtype=dtype) for k, v in out.items()}
    if mode == "normal_dep":
        out["normal_dep"] = (depth2normal(out["depth"]) + 1) / 2
    img = out[mode]
    if mode in ("depth", "alpha"):
        img = img.repeat(3, 1, 1)
        if mode == "depth":
            img = (img - img.min()) / (img.max() - img.min() + 1e-20)
    img = torch.nn.functional.interpolate(img.unsqueeze(0), size=size, mode="bilinear", align_corners=False).squeeze(0)
    return img.permute(1, 2, 0).contiguous().clamp(0, 1).double().numpy()


def frames():
    kw = {}
    for name, shape, kind in VR.D2N_CASES:
        d = VR.make_depth(shape, kind)
        n64 = depth2normal(torch.tensor(d, dtype=torch.float64)).numpy()
        n32 = depth2normal(torch.tensor(d, dtype=torch.float32)).double().numpy()
        assert np.isfinite(n64).all() and np.isfinite(n32).all()
        kw["normal_" + name], kw["dev32_d2n_" + name] = n64, np.float64(np.abs(n32 - n64).max())
        ours = VR.depth2normal(d)
        print("%-28s dev32 %.3g   restatement - reference %.3g" % (name, kw["dev32_d2n_" + name], np.abs(ours - n64).max()))
    for name, mode, case, size in VR.FRAME_CASES:
        out = VR.make_out(case)
        f64, f32 = reference_frame(out, mode, size, torch.float64), reference_frame(out, mode, size, torch.float32)
        kw["dev32_" + name] = np.float64(np.abs(f32 - f64).max())
        ours = VR.display_frame(out, mode, size)
        print("%-28s dev32 %.3g   restatement - reference %.3g" % (name, kw["dev32_" + name], np.abs(ours - f64).max()))
    save("viewer_frames", seed=np.int64(VR.SEED), **kw)


# --------------------------------------------------------------------------- overlays
def _calls():
    got = list(CALLS)
    CALLS.clear()
    return got


def _poly(calls):
    """(pts (n, 2, 2) or (n, S, 2), colours (n, 3), thickness) of the COLOUR layer's polylines: each is drawn twice, alpha first."""
    c = [k for kind, a, k in calls if kind == "polylines"]
    alpha, colour = c[0::2], c[1::2]
    assert all(list(k["color"]) == [1, 1, 1] for k in alpha) and len(alpha) == len(colour)
    assert all(np.array_equal(x["pts"][0], y["pts"][0]) and x["thickness"] == y["thickness"] for x, y in zip(alpha, colour))
    assert all(k["pts"][0].dtype == np.int32 and not k["isClosed"] for k in colour)
    return (np.stack([k["pts"][0] for k in colour]), np.float64([k["color"] for k in colour]), np.int64(colour[0]["thickness"]))


def _circles(calls):
    c = [k for kind, a, k in calls if kind == "circle"]
    alpha, colour = c[0::2], c[1::2]
    assert all(np.array_equal(x["center"], y["center"]) and x["thickness"] == y["thickness"] == -1 for x, y in zip(alpha, colour))
    return (np.stack([k["center"] for k in colour]), np.float64([k["color"] for k in colour]), np.int64(colour[0]["radius"]),
            np.int64(alpha[0]["radius"]))


def _order(calls):
    return "".join({"polylines": "p", "circle": "c", "rectangle": "r"}[kind] for kind, a, k in calls)


def scene(seed):
    """The overlay scene of one seed, or None where a coordinate that the tests compare sits within 1e-3 px of an integer (rounding
    must not decide a pixel)."""
    H, W = 60, 90  # (not square: the editor's x is scaled by the height)
    g = torch.Generator().manual_seed(seed)
    cam = synth.look_at_camera(H, W, azimuth_deg=35.0, elevation_deg=15.0, radius=3.0)
    Kmat = torch.tensor([[110.0, 0, 41.5], [0, 108.0, 33.25], [0, 0, 1]])
    camK = types.SimpleNamespace(**{**cam.__dict__, "K": Kmat})
    cam = types.SimpleNamespace(**{**cam.__dict__, "K": None})
    joints, parents = synth.make_skeleton(g, 24)
    d_nodes = (joints + 0.03 * torch.randn(24, 3, generator=g)).contiguous()
    ref_nodes = torch.tensor([[-0.4, 0.5, 0.1], [0.0, 0.1, 0.0], [0.5, -0.3, -0.2]]) + 0.01 * torch.randn(3, 3, generator=g)
    ref_parents = torch.tensor([-1, 0, 1])
    G, S_cap, pushes = 8, 5, 7
    cloud = 0.6 * torch.randn(40, 3, generator=g)
    traj_idx = torch.randperm(40, generator=g)[:G]
    steps = [cloud + 0.05 * k * torch.randn(40, 3, generator=g) for k in range(pushes)]
    kpt = 5
    kw = dict(seed=np.int64(seed), H=np.int64(H), W=np.int64(W), full_proj=cam.full_proj_transform.numpy(),
              world_view=cam.world_view_transform.numpy(), FoVx=np.float64(cam.FoVx), FoVy=np.float64(cam.FoVy), K=Kmat.numpy(),
              joints=joints.numpy(), parents=parents.numpy(), d_nodes=d_nodes.numpy(), ref_nodes=ref_nodes.numpy(),
              ref_parents=ref_parents.numpy(), traj_idx=traj_idx.numpy(), traj_steps=torch.stack(steps).numpy(), keypoint=np.int64(kpt))
    margins = []
    uv, ok = VR.project_editor(d_nodes.numpy(), kw["full_proj"], H, W)
    r_sq = int((H + W) / 2 * 0.005)
    margins += [VR.margin(uv, ok) if ok.all() else 0.0, VR.margin(uv[kpt:kpt + 1], ok[kpt:kpt + 1], (-r_sq, r_sq))]
    uvr, okr = VR.project_editor(ref_nodes.numpy(), kw["full_proj"], H, W)
    margins.append(VR.margin(uvr, okr) if okr.all() else 0.0)
    tr = torch.stack(steps)[-S_cap:, traj_idx].numpy()
    uvt, okt = VR.project_editor(tr.reshape(-1, 3), kw["full_proj"], H, W)
    margins.append(VR.margin(uvt, okt) if okt.all() else 0.0)
    for c in (cam, camK):
        uvk, okk = VR.project_render_rig(d_nodes.numpy(), kw["world_view"], c.FoVx, c.FoVy, H, W, None if c.K is None else c.K.numpy())
        margins.append(VR.margin(uvk, okk) if okk.all() else 0.0)
    if min(margins) < 1e-3:
        return None
    return kw, cam, camK, (joints, parents, d_nodes, ref_nodes, ref_parents, G, S_cap, pushes, traj_idx, steps, kpt)


def overlays():
    found = next(s for s in (scene(VR.SEED + k) for k in range(64)) if s is not None)
    kw, cam, camK, (joints, parents, d_nodes, ref_nodes, ref_parents, G, S_cap, pushes, traj_idx, steps, kpt) = found
    H, W = int(kw["H"]), int(kw["W"])
    g = torch.Generator().manual_seed(int(kw["seed"]) + 1000)
    print("overlay scene: seed", int(kw["seed"]))

    GUI = interactive_GUI.GUI
    deform = types.SimpleNamespace(parents=parents, nodes=torch.cat([joints, torch.zeros(24, 8)], 1))
    me = types.SimpleNamespace(skeleton=types.SimpleNamespace(deform=deform))
    with S.quiet():
        GUI.update_skeleton_edges(me, cam, d_nodes, thickness=2)
    calls = _calls()
    assert _order(calls) == "pp" * 23 + "cc" * 24
    kw["skel_edges"], kw["skel_edge_colors"], kw["skel_thickness"] = _poly(calls)
    kw["skel_centers"], kw["skel_disc_colors"], kw["skel_color_radius"], kw["skel_alpha_radius"] = _circles(calls)

    me = types.SimpleNamespace(update_reference_skeleton_edited_pos=lambda: (ref_nodes, ref_parents))
    with S.quiet():
        GUI.update_reference_skeleton(me, cam, thickness=2)
    calls = _calls()
    assert _order(calls) == "cc" * 3 + "pp" * 2  # the discs first
    kw["ref_edges"], kw["ref_edge_colors"], kw["ref_thickness"] = _poly(calls)
    kw["ref_centers"], kw["ref_disc_colors"], kw["ref_color_radius"], kw["ref_alpha_radius"] = _circles(calls)

    from matplotlib import cm
    me = types.SimpleNamespace(traj_coor=torch.zeros([0, G, 4]), traj_idx=traj_idx, traj_color_map=cm.get_cmap("jet"))
    for k in range(pushes):
        _calls()
        with S.quiet():
            GUI.update_trajectory_overlay(me, steps[k], cam, samp_num=S_cap, gs_num=G, thickness=1)
    calls = _calls()
    assert _order(calls) == "pp" * G
    kw["traj_pts"], kw["traj_colors"], kw["traj_thickness"] = _poly(calls)
    assert kw["traj_pts"].shape == (G, S_cap, 2)

    kp = types.SimpleNamespace(get_kpt=lambda: [0], get_kpt_idx=lambda: [kpt])
    me = types.SimpleNamespace(need_update_overlay=True, deform_keypoints=kp, animation_deform_nodes=d_nodes, edit_reference_skeleton=False,
                               buffer_image=np.zeros((H, W, 3), np.float32), cur_cam=cam, H=H, W=W, buffer_overlay=None)
    with S.quiet():
        GUI.update_control_point_overlay(me)
    calls = _calls()
    assert _order(calls) == "r" and me.buffer_overlay is not None
    (_, a, k), = calls
    kw["square_lt"], kw["square_rb"], kw["square_color"] = np.int64(a[0]), np.int64(a[1]), np.float64(k["color"])
    assert k["thickness"] == -1

    rgba = torch.rand(4, H, W, generator=g)
    for tag, c in (("rr", cam), ("rrK", camK)):
        with S.quiet():
            render_rig.project_nodes_to_2d_withnodes(c, None, d_nodes, parents, rgba, "unused.png", thickness=1)
        calls = _calls()
        assert _order(calls) == "pp" * 23 + "cc" * 24
        kw[tag + "_edges"], kw[tag + "_edge_colors"], kw[tag + "_thickness"] = _poly(calls)
        kw[tag + "_centers"], kw[tag + "_disc_colors"], kw[tag + "_color_radius"], kw[tag + "_alpha_radius"] = _circles(calls)
    save("viewer_overlays", **kw)

    jet = cm.get_cmap("jet")
    save("viewer_jet512", colors=np.array([np.array(jet(i / max(1, float(512 - 1)))[:3]) * 255 for i in range(512)], dtype=np.int32) / 255)


if __name__ == "__main__":
    torch.set_num_threads(1)
    frames()
    overlays()
