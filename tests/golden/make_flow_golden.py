"""Fixtures of the optical-flow term from the reference Python on the CPU (tests/golden/_ref_shim.py, unchanged): the
reference's own ``gaussian_renderer.render_flow`` is called with the shim's capturing rasterizer.

  flow_<case>.npz      inputs, the captured means3D / colors_precomp / opacities / scales / rotations / cov3D_precomp and
                       settings, the gradients of a seeded cotangent on colors_precomp w.r.t. d_xyz1, d_xyz2 and feature,
                       and ``colour_ref_err`` / ``grad_ref_err``: the largest error of the reference's float32 colours and of
                       its three gradients against tests/flow_ref.py in float64 on the same float32 inputs (a measurement
                       of the reference)
  flow_loss_ref.npz    the statements train_gui.py:1101-1105 and :1112-1120 executed as they stand (read from the reference
                       at generation time, never copied) on seeded inputs: the loss and its gradient to the rendered motion
  flow_landmarks.json  landmark_interpolate at the default lambda_optical landmarks, steps 0 .. 25 001

Every point of every case keeps h.w >= 0.5 for both cameras (asserted), so the reference is finite everywhere.
"""
import json
import math
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim as S  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import flow_ref as FR  # noqa: E402

CASES = {
    # name: (seed, N, motion mask, isotropic, second camera, d_rotation1 as float, scale_const, d_rot_as_res, cov python, K)
    "mask_aniso": dict(seed=41, N=300, mask=True, iso=False),
    "nomask_iso": dict(seed=42, N=257, mask=False, iso=True),
    "one_camera": dict(seed=43, N=200, mask=True, iso=False, cam2=False),
    "float_rotation": dict(seed=44, N=200, mask=True, iso=True, d_rot_float=True),
    "scale_const": dict(seed=45, N=200, mask=False, iso=False, scale_const=0.03),
    "quat_product": dict(seed=46, N=200, mask=True, iso=False, d_rot_as_res=False),
    "cov_python": dict(seed=47, N=200, mask=True, iso=False, cov_python=True),
    "principal_point_K": dict(seed=48, N=300, mask=True, iso=False, from_K=True),
}


def np_(t):
    return t.detach().cpu().numpy().astype(np.float32)


def camera(Camera, az, el, rad, H, W, fid, from_K):
    az, el = math.radians(az), math.radians(el)
    eye = np.array([rad * math.cos(el) * math.sin(az), -rad * math.sin(el), -rad * math.cos(el) * math.cos(az)])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(np.array([0.0, -1.0, 0.0]), fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    R = np.stack([right, up, fwd], axis=1)
    T = -R.T @ eye
    fov = 0.6911112
    K = None
    if from_K:
        fx = W / (2 * math.tan(fov / 2))
        K = np.array([[fx, 0, W / 2 + 13.0 * W / 1024], [0, fx, H / 2 - 7.0 * H / 1024], [0, 0, 1]], dtype=np.float64)
    return Camera(0, R, T, fov, fov * 0.8, torch.zeros(3, H, W), None, "c", 0, data_device="cpu", fid=fid, K=K)


def fixture(name, seed, N, mask, iso, cam2=True, d_rot_float=False, scale_const=None, d_rot_as_res=True, cov_python=False,
            from_K=False):
    with S.quiet():
        from gaussian_renderer import render_flow
        from scene.gaussian_model import GaussianModel
        from scene.cameras import Camera
    g = torch.Generator().manual_seed(seed)
    P = torch.nn.Parameter
    gm = GaussianModel(3, fea_dim=4, with_motion_mask=mask, use_isotropic_gs=iso)
    gm._xyz = P(0.6 * torch.randn(N, 3, generator=g))
    gm._features_dc = P(torch.randn(N, 1, 3, generator=g))
    gm._features_rest = P(0.1 * torch.randn(N, 15, 3, generator=g))
    gm._scaling = P(math.log(0.05) + 0.35 * torch.randn(N, 1 if iso else 3, generator=g))
    gm._rotation = P(torch.randn(N, 4, generator=g))
    gm._opacity = P(1.5 * torch.randn(N, 1, generator=g))
    gm.feature = P(torch.randn(N, gm.fea_dim, generator=g))
    H, W = 40, 56
    c1 = camera(Camera, 45.0, 20.0, 4.0, H, W, 0.37, from_K)
    c2 = camera(Camera, 52.0, 16.0, 4.3, H, W, 0.41, from_K) if cam2 else None
    d1 = (0.05 * torch.randn(N, 3, generator=g)).requires_grad_(True)
    d2 = (0.05 * torch.randn(N, 3, generator=g)).requires_grad_(True)
    d_rot = 0.0 if d_rot_float else (torch.tensor([1.0, 0, 0, 0]) * (0.0 if d_rot_as_res else 1.0)
                                     + 0.1 * torch.randn(N, 4, generator=g))
    d_scaling = 0.01 * torch.rand(N, 3, generator=g)
    cot = torch.randn(N, 3, generator=g)
    # h.w >= 0.5 for both cameras
    for d, c in ((d1, c1), (d2, c2 if c2 is not None else c1)):
        hw = torch.cat([gm._xyz + d, torch.ones(N, 1)], -1).detach() @ c.full_proj_transform
        assert float(hw[:, 3].min()) >= 0.5, (name, float(hw[:, 3].min()))
    render_flow(gm, c1, c2, d1, d2, d_rot, d_scaling, scaling_modifier=1.0, compute_cov3D_python=cov_python,
                scale_const=scale_const, d_rot_as_res=d_rot_as_res)
    kw, st = S.CAPTURE["kwargs"], S.CAPTURE["settings"]
    col = kw["colors_precomp"]
    wrt = [d1, d2] + ([gm.feature] if mask else [])
    grads = torch.autograd.grad((col * cot).sum(), wrt)
    F2 = (c2 if c2 is not None else c1).full_proj_transform
    ref64 = FR.colours(gm._xyz.double(), d1.double(), d2.double(), c1.full_proj_transform.double(), F2.double(),
                       torch.sigmoid(gm.feature.double()[:, -1:]) if mask else None)
    ref_err = float((col.detach().double() - ref64.detach()).abs().max())
    d1_64, d2_64, fe64 = (t.detach().double().requires_grad_(True) for t in (d1, d2, gm.feature))
    col64 = FR.colours(gm._xyz.double(), d1_64, d2_64, c1.full_proj_transform.double(), F2.double(),
                       torch.sigmoid(fe64[:, -1:]) if mask else None)
    g64 = torch.autograd.grad((col64 * cot.double()).sum(), [d1_64, d2_64] + ([fe64] if mask else []))
    grad_err = [float((a.double() - b).abs().max()) for a, b in zip(grads, g64)] + ([] if mask else [0.0])
    none = np.zeros((0,), np.float32)
    opt = lambda k: np_(kw[k]) if kw[k] is not None else none  # noqa: E731
    z = dict(
        xyz=np_(gm._xyz), scaling=np_(gm._scaling), rotation=np_(gm._rotation), opacity=np_(gm._opacity), feature=np_(gm.feature),
        with_motion_mask=np.bool_(mask), isotropic=np.bool_(iso), d_xyz1=np_(d1), d_xyz2=np_(d2),
        d_rotation1=(none if d_rot_float else np_(d_rot)), d_rotation_is_float=np.bool_(d_rot_float), d_scaling1=np_(d_scaling),
        scale_const=np.float64(-1.0 if scale_const is None else scale_const), d_rot_as_res=np.bool_(d_rot_as_res),
        compute_cov3D_python=np.bool_(cov_python), has_camera2=np.bool_(c2 is not None), cotangent=np_(cot),
        view1=np_(c1.world_view_transform), proj1=np_(c1.full_proj_transform), campos1=np_(c1.camera_center),
        proj2=np_(F2), fovx=np.float64(c1.FoVx), fovy=np.float64(c1.FoVy), H=np.int64(H), W=np.int64(W),
        means3D=np_(kw["means3D"]), colors_precomp=np_(col), opacities=np_(kw["opacities"]), scales=opt("scales"),
        rotations=opt("rotations"), cov3D_precomp=opt("cov3D_precomp"), shs_is_none=np.bool_(kw["shs"] is None),
        bg=np_(st.bg), sh_degree=np.int64(st.sh_degree), viewmatrix=np_(st.viewmatrix), projmatrix=np_(st.projmatrix),
        campos=np_(st.campos), tanfovx=np.float64(st.tanfovx), tanfovy=np.float64(st.tanfovy),
        image_height=np.int64(st.image_height), image_width=np.int64(st.image_width), scale_modifier=np.float64(st.scale_modifier),
        grad_d_xyz1=np_(grads[0]), grad_d_xyz2=np_(grads[1]), grad_feature=(np_(grads[2]) if mask else none),
        colour_ref_err=np.float64(ref_err), grad_ref_err=np.float64(grad_err))
    np.savez_compressed(os.path.join(HERE, "flow_" + name + ".npz"), **z)
    print("wrote flow_" + name, "N", N, "reference's own colour error vs float64: %.3g" % ref_err)


def fixture_loss(name, seed, C, H, W, mask_channels):
    """train_gui.py:1101-1105 and :1112-1120 as they stand in the reference, executed on seeded inputs."""
    with S.quiet():
        from utils.loss_utils import l1_loss
    lines = open(os.path.join(S.REF, "train_gui.py")).read().split("\n")
    picked = lines[1100:1105] + lines[1111:1120]
    assert "coor1to2_flow = flow /" in picked[0] and "optical_flow_loss = l1_loss(" in picked[-1], (picked[0], picked[-1])
    g = torch.Generator().manual_seed(seed)
    image, gt_image = torch.rand(C, H, W, generator=g), torch.rand(C, H, W, generator=g)
    motion = (0.2 * torch.randn(3, H, W, generator=g)).requires_grad_(True)
    alpha = torch.rand(1, H, W, generator=g) * 0.3 + 0.75
    flow = 8.0 * torch.randn(H, W, 2, generator=g)
    masks = (torch.rand(H, W, mask_channels, generator=g) > 0.45).float()
    fid1, fid2 = torch.tensor([0.30]), torch.tensor([0.55])
    ns = dict(torch=torch, np=np, l1_loss=l1_loss, flow=flow, masks=masks, image=image, gt_image=gt_image, fid1=fid1, fid2=fid2,
              render_pkg2={"render": motion, "alpha": alpha})
    exec(textwrap.dedent("\n".join(picked)), ns)
    loss = ns["optical_flow_loss"]
    grad, = torch.autograd.grad(loss, motion)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), image=np_(image), gt=np_(gt_image), motion=np_(motion), alpha=np_(alpha),
                        flow=np_(flow), masks=np_(masks), fid1=np_(fid1), fid2=np_(fid2), loss=np.float32(loss.item()),
                        grad_motion=np_(grad), weight=np_(ns["mask"][..., 0]))
    print("wrote", name, "loss", loss.item(), "live", float((ns["mask"] != 0).float().mean()))


def landmarks(path):
    with S.quiet():
        from utils.time_utils import landmark_interpolate
    lm, st = [1e-1, 1e-1, 1e-3, 0], [0, 15_000, 25_000, 25_001]  # arguments/__init__.py:153-154
    steps = [0, 1, 7_499, 14_999, 15_000, 15_001, 17_500, 20_000, 22_222, 24_999, 25_000, 25_001, 25_002, 40_000]
    out = {"landmarks": lm, "steps": st, "at": steps,
           "log": [float(landmark_interpolate(lm, st, s)) for s in steps],
           "linear": [float(landmark_interpolate(lm, st, s, interpolation="linear")) for s in steps]}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    S.install()
    for name, kw in CASES.items():
        fixture(name, **kw)
    fixture_loss("flow_loss_ref", 51, 3, 24, 40, 3)
    landmarks(os.path.join(HERE, "flow_landmarks.json"))
