"""Restatement of the optical-flow term of a stage-1 iteration, in torch, in whatever dtype and on whatever device its inputs
have: float64 on the CPU it is what the HIP kernels (riggs_amd/csrc/flow.hip) are pinned to; float32 on the GPU it is the
"torch-op form" a user of the reference runs over the drop-in rasterizer (tools/flow_time.py times it).

  colours(...)           gaussian_renderer.render_flow, gaussian_renderer/__init__.py:186-202
  render_flow_glue(...)  what render_flow hands to the rasterizer besides the colours, :221-246
  flow_loss(...)         train_gui.py:1101-1120 (inline in the trainer's step: there is no callable to import)

Written from the formulas, in the reference's order of operations; tests/golden/make_flow_golden.py records what the
reference's own render_flow computes and tests/test_flow_cpu.py holds this file to it.  ``fault=`` plants one of four
deliberate errors, for the tests that show the bounds below reject them.

Error bounds (u0 = 2^-24 is the unit roundoff of float32, eps = 2 u0 its machine epsilon) — all derived from the kernels'
operation counts, none from what the kernels give:

Colours.  p = x + d is one rounding; h_j = ((p_x F_0j + p_y F_1j) + p_z F_2j) + F_3j is three products and three sums of
operands that carry p's rounding, so |dh_j| <= 5 u0 S_j with S_j = sum of the |terms| (the usual gamma_n bound, first order);
u = h_x / h_w is one correctly rounded division: |du| <= u0 (|u| + 5 S_x / |h_w| + 5 |u| S_w / |h_w|).  The colour is
fl(u2 - u1): another u0 (|u1| + |u2|).  The bound is per element because the flow is a difference of two nearly equal screen
coordinates: relative to the flow it means nothing, relative to eps max(|u1|, |u2|, 1) it is the small multiple
(2 + 5 S_x / |h_x| + 5 S_w / |h_w|) / 2 per camera — 6 where nothing cancels inside h.  The mask is
1 / (1 + expf(-l)): expf to 1 ulp (2 u0), a sum, a division: 4 u0 m.

Colour gradients.  dL/dh = (g_x / w, g_y / w, ., -(g_x u_x + g_y u_y) / w) and dL/dp_i = F_i0 dh_x + F_i1 dh_y + F_i3 dh_w,
from the recomputed u and w: w carries 5 u0 S_w, u the bound above; each quotient and product adds its u0.  The Jacobian
scales with 1 / w, and so does the bound.

Loss.  The weight w = live * pair * cos(mean_c |image - gt| pi / 2): the cosine's argument is 2 C roundings of the mean, the
rounded 1 / C and pi / 2 and two products (<= (C + 4) u0 relative, argument <= pi / 2), cosf is good to 1 ulp: together
(1.571 (C + 4) + 2) u0 absolute; pair: 1.571 * 3 + 2 -> 7 u0; one product: |dw| <= W_OPS(C) u0 live pair.  A term
|w c - w m| adds c's division and the two products' and the difference's roundings: 3 more.  The sum is 8 additions in a
thread, 6 across the wave, 2 across the workgroup in float32 (depth 16), the rest in float64.  So
  |loss - restatement| <= u0 (W_OPS + 3 + 16) sum(live pair (|c| + |m|)) / (2 H W).
Loss gradient: -sign(w c - w m) w / (2 H W).  Where |w (c - m)| is below the rounding of the two products and of c,
4 u0 w (|c| + |m|), the sign is undecidable and the pixel is excluded; elsewhere |dg| <= u0 (W_OPS + 3) live pair / (2 H W).
"""
import math

import torch

U0 = 2.0 ** -24
EPS = 2.0 ** -23
FAULTS = ("swap_F2", "w_eps", "normalise_after_add", "alpha_half")


def w_ops(C):
    return math.ceil(1.571 * (C + 4) + 2) + 7 + 1


# ---- colours --------------------------------------------------------------------------------------------------------------
def _project(p, F, w_eps=0.0):
    h = torch.cat([p, torch.ones_like(p[..., :1])], dim=-1) @ F
    return h[..., :3] / (h[..., -1:] + w_eps), h


def colours(xyz, d_xyz1, d_xyz2, F1, F2, motion_mask, fault=None):
    """(N, 3): screen-space motion from (xyz + d_xyz1 seen through F1) to (xyz + d_xyz2 seen through F2), the motion mask in
    the third column.  xyz is a constant; F2 None = F1; the residuals may be 0.0; motion_mask (N, 1) or None (= 1)."""
    x = xyz.detach()
    F2 = F1 if (F2 is None or fault == "swap_F2") else F2
    e = 1e-7 if fault == "w_eps" else 0.0
    u1, _ = _project(x + d_xyz1, F1, e)
    u2, _ = _project(x + d_xyz2, F2, e)
    flow = u2 - u1
    m = torch.ones_like(x[..., :1]) if motion_mask is None else motion_mask
    return torch.cat([flow[..., :2], m], dim=-1)


def colour_bounds(xyz, d_xyz1, d_xyz2, F1, F2, logit=None, g=None):
    """Per-element bounds of the kernel's colours (N, 3) — and, with a cotangent ``g`` (N, 3), of its three gradients —
    against ``colours`` evaluated in float64 on the same float32 inputs.  Everything here is float64."""
    x = xyz.double()
    F2 = F1 if F2 is None else F2
    out = {}
    cams = []
    for d, F in ((d_xyz1, F1), (d_xyz2, F2)):
        F = F.double()
        p = x + (d.double() if isinstance(d, torch.Tensor) else 0.0)
        h = torch.cat([p, torch.ones_like(p[:, :1])], -1) @ F
        S = torch.cat([p, torch.ones_like(p[:, :1])], -1).abs() @ F.abs()
        w = h[:, 3:4]
        u = h[:, :2] / w
        rw = 5 * S[:, 3:4] / w.abs()                                   # relative error of w, in u0
        ru = u.abs() + 5 * S[:, :2] / w.abs() + u.abs() * rw           # absolute error of u, in u0
        cams.append((F, u, w, rw, ru))
    (_, u1, _, _, ru1), (_, u2, _, _, ru2) = cams
    m = torch.ones_like(x[:, :1]) if logit is None else torch.sigmoid(logit.double().reshape(-1, 1))
    out["colour"] = U0 * torch.cat([ru1 + ru2 + u1.abs() + u2.abs(), 4 * m], -1)
    out["units"] = out["colour"][:, :2] / (EPS * torch.maximum(torch.maximum(u1.abs(), u2.abs()), torch.ones_like(u1)))
    if g is not None:
        g = g.double()
        gx, gy = g[:, 0:1], g[:, 1:2]
        for name, (F, u, w, rw, ru) in zip(("d_xyz1", "d_xyz2"), cams):
            ghx, ghy = gx / w, gy / w
            t_abs = (gx * u[:, 0:1]).abs() + (gy * u[:, 1:2]).abs()
            ghw = (gx * u[:, 0:1] + gy * u[:, 1:2]) / w
            e_hx, e_hy = ghx.abs() * (1 + rw), ghy.abs() * (1 + rw)
            e_t = 2 * t_abs + gx.abs() * ru[:, 0:1] + gy.abs() * ru[:, 1:2]
            e_hw = e_t / w.abs() + ghw.abs() * (1 + rw)
            Fa = F.abs()[:3]                                           # rows i = 0..2, columns (0, 1, 3)
            terms = Fa[:, 0] * ghx.abs() + Fa[:, 1] * ghy.abs() + Fa[:, 3] * ghw.abs()
            out[name] = U0 * (3 * terms + Fa[:, 0] * e_hx + Fa[:, 1] * e_hy + Fa[:, 3] * e_hw)
        out["logit"] = U0 * g[:, 2].abs() * (7 * m * (1 - m) + 4 * m * m)[:, 0]
    return out


# ---- the glue of render_flow ----------------------------------------------------------------------------------------------
def quaternion_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    o = torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)
    return torch.where(o[..., 0:1] < 0, -o, o)


def _raw_multiply(a, b):  # scene/gaussian_model.py:25-34 (not standardised)
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def covariance6(scales, modifier, rotation):
    q = rotation / rotation.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1).reshape(-1, 3, 3)
    M = R * (modifier * scales)[:, None, :]
    S = M @ M.transpose(1, 2)
    return torch.stack((S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]), -1)


def render_flow_glue(xyz, scaling, rotation, opacity, isotropic, d_xyz1, d_rotation1, d_scaling1, scaling_modifier=1.0,
                     compute_cov3D_python=False, scale_const=None, d_rot_as_res=True, fault=None):
    """means3D, opacities, scales, rotations, cov3D_precomp as render_flow hands them to the rasterizer, from the raw
    parameters (``scaling`` is (N, 1) or (N, 3) raw; isotropic repeats its first column)."""
    get_scaling = torch.exp(scaling[..., :1].repeat(1, 3) if isotropic else scaling)
    get_rotation = torch.nn.functional.normalize(rotation)

    def rotated():
        if d_rot_as_res:
            if fault == "normalise_after_add":
                return torch.nn.functional.normalize(rotation + d_rotation1)
            return get_rotation + d_rotation1
        return get_rotation if type(d_rotation1) is float else quaternion_multiply(d_rotation1, get_rotation)
    out = {"means3D": xyz + d_xyz1, "opacities": torch.sigmoid(opacity), "scales": None, "rotations": None, "cov3D_precomp": None}
    if scale_const is not None:
        out["scales"], out["rotations"] = torch.ones_like(get_scaling) * scale_const, rotated()
    elif compute_cov3D_python:
        r = rotation if type(d_rotation1) is float else _raw_multiply(rotation, d_rotation1)
        out["cov3D_precomp"] = covariance6(get_scaling, scaling_modifier, r)
    else:
        out["scales"], out["rotations"] = get_scaling + d_scaling1, rotated()
    return out


# ---- the loss -------------------------------------------------------------------------------------------------------------
def flow_weight(image, gt, alpha, masks, fid1, fid2, fault=None):
    thr = 0.5 if fault == "alpha_half" else 0.9
    live = (alpha.reshape(alpha.shape[-2:]) > thr) & ((masks[..., 0] > 0) | (masks[..., 1] > 0))
    df = torch.as_tensor(fid1, dtype=image.dtype, device=image.device) - torch.as_tensor(fid2, dtype=image.dtype, device=image.device)
    pair = torch.clamp(torch.cos(df.abs().reshape(()) * math.pi / 2), 0.2, 1)
    l1w = torch.cos((image.detach() - gt).abs().mean(dim=0) * math.pi / 2)
    return live * pair * l1w, live * pair


def flow_loss(image, gt, motion, alpha, flow, masks, fid1, fid2, fault=None):
    """The scalar of train_gui.py:1120; differentiable w.r.t. ``motion`` (3, H, W)."""
    H, W = motion.shape[1:]
    c = flow / torch.tensor([W, H], dtype=flow.dtype, device=flow.device) * 2
    w = flow_weight(image, gt, alpha.detach(), masks, fid1, fid2, fault)[0][..., None]
    m = motion[:2].permute(1, 2, 0)
    return (w * c - w * m).abs().mean()


def flow_loss_parts(image, gt, motion, alpha, flow, masks, fid1, fid2):
    """float64: loss, dL/dmotion (3, H, W), the bound of the loss, the per-pixel bound of the gradient (H, W), the (H, W, 2)
    mask of undecidable signs, and the live mask."""
    d = lambda t: t.double() if isinstance(t, torch.Tensor) else t  # noqa: E731
    image, gt, alpha, flow, masks, fid1, fid2 = map(d, (image, gt, alpha, flow, masks, fid1, fid2))
    motion = motion.double().detach().requires_grad_(True)
    loss = flow_loss(image, gt, motion, alpha, flow, masks, fid1, fid2)
    grad, = torch.autograd.grad(loss, motion)
    H, W = motion.shape[1:]
    C = image.shape[0]
    w, gross = flow_weight(image, gt, alpha, masks, fid1, fid2)
    c = flow / torch.tensor([W, H], dtype=flow.dtype) * 2
    m = motion.detach()[:2].permute(1, 2, 0)
    mag = c.abs() + m.abs()
    loss_bound = U0 * (w_ops(C) + 3 + 16) * float((gross[..., None] * mag).sum()) / (2 * H * W)
    grad_bound = U0 * (w_ops(C) + 3) * gross / (2 * H * W)
    undecidable = ((w[..., None] * (c - m)).abs() < 4 * U0 * w.abs()[..., None] * mag) & (gross > 0)[..., None]
    return loss.detach(), grad, loss_bound, grad_bound, undecidable, gross > 0


# ---- comparisons the CPU and the GPU tests share ---------------------------------------------------------------------------
def colour_ratio(got, xyz, d_xyz1, d_xyz2, F1, F2, logit=None, extra=0.0):
    """Worst |got - float64 restatement| / bound over the (N, 3) colours ``got`` (<= 1 passes), and the worst error of the two
    flow columns in units of eps max(|u1|, |u2|, 1).  ``extra``: an absolute allowance on top (the reference's own measured
    error, when ``got`` is compared through a float32 fixture)."""
    d = lambda t: t.detach().double().cpu() if isinstance(t, torch.Tensor) else t  # noqa: E731
    xyz, d_xyz1, d_xyz2, F1, F2, logit = map(d, (xyz, d_xyz1, d_xyz2, F1, F2, logit))
    if xyz.shape[0] == 0:
        return 0.0, 0.0
    want = colours(xyz, d_xyz1, d_xyz2, F1, F2, None if logit is None else torch.sigmoid(logit.reshape(-1, 1)))
    b = colour_bounds(xyz, d_xyz1, d_xyz2, F1, F2, logit)
    err = (d(got) - want).abs()
    unit = b["colour"][:, :2] / b["units"]
    return float((err / (b["colour"] + extra)).max()), float((err[:, :2] / unit).max())


def colour_grad_ratios(got, g, xyz, d_xyz1, d_xyz2, F1, F2, logit=None, extra=(0.0, 0.0, 0.0)):
    """Worst |got - float64 autograd of the restatement| / bound for ``got = (dL/dd_xyz1, dL/dd_xyz2, dL/dlogit)`` (entries may
    be None) under the cotangent ``g`` (N, 3)."""
    d = lambda t: t.detach().double().cpu() if isinstance(t, torch.Tensor) else t  # noqa: E731
    xyz, F1, F2, g = map(d, (xyz, F1, F2, g))
    N = xyz.shape[0]
    if N == 0:
        return [0.0, 0.0, 0.0]
    leaf = lambda t: (d(t) if isinstance(t, torch.Tensor) else torch.zeros(N, 3, dtype=torch.float64)).requires_grad_(True)  # noqa: E731
    a1, a2 = leaf(d_xyz1), leaf(d_xyz2)
    lg = None if logit is None else d(logit).reshape(-1).requires_grad_(True)
    col = colours(xyz, a1, a2, F1, F2, None if lg is None else torch.sigmoid(lg[:, None]))
    want = torch.autograd.grad((col * g).sum(), [a1, a2] + ([lg] if lg is not None else []))
    b = colour_bounds(xyz, a1.detach(), a2.detach(), F1, F2, None if lg is None else lg.detach(), g)
    out = []
    for i, name in enumerate(("d_xyz1", "d_xyz2", "logit")):
        if got[i] is None or i >= len(want):
            out.append(0.0)
            continue
        err, bound = (d(got[i]).reshape(want[i].shape) - want[i]).abs(), b[name] + extra[i]
        ok = (err == 0) & (bound == 0)  # (a zero cotangent row: exact zeros on both sides)
        out.append(float(torch.where(ok, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max()))
    return out


def loss_ratios(loss, grad, image, gt, motion, alpha, flow, masks, fid1, fid2):
    """(|loss - restatement| / bound, worst gradient error / bound over the decidable pixels, share of the live pixels whose
    sign is undecidable) for the kernel's ``loss`` (scalar) and ``grad`` (3, H, W), the restatement fed the same float32
    tensors."""
    c = lambda t: t.detach().cpu() if isinstance(t, torch.Tensor) else t  # noqa: E731
    want, wgrad, lb, gb, und, live = flow_loss_parts(*map(c, (image, gt, motion, alpha, flow, masks, fid1, fid2)))
    r_loss = abs(float(c(loss)) - float(want)) / lb if lb > 0 else (0.0 if float(c(loss)) == float(want) else float("inf"))
    r_grad = 0.0
    if grad is not None:
        err = (c(grad).double() - wgrad).abs()
        assert float(err[2].max()) == 0.0, "the gradient's third plane must be zero"
        e2 = err[:2].permute(1, 2, 0)
        dec = ~und
        exact = (e2 == 0)
        ratio = torch.where(exact, torch.zeros_like(e2), e2 / gb[..., None].clamp_min(1e-300))
        r_grad = float(ratio[dec].max()) if bool(dec.any()) else 0.0
    n_live = int(live.sum())
    share = float(und.any(-1).sum()) / n_live if n_live else 0.0
    return r_loss, r_grad, share


def load_fixture(path):
    """A flow_<case>.npz as a dict of torch tensors / Python scalars."""
    import numpy as np
    z = np.load(path)
    out = {}
    for k in z.files:
        v = z[k]
        out[k] = (v.item() if v.ndim == 0 else torch.from_numpy(v))
    return out


def fixture_glue_args(z, device="cpu"):
    """The keyword arguments render_flow saw in a fixture (beyond the Gaussians and cameras)."""
    t = lambda k: z[k].to(device)  # noqa: E731
    return dict(d_xyz1=t("d_xyz1"), d_rotation1=0.0 if z["d_rotation_is_float"] else t("d_rotation1"), d_scaling1=t("d_scaling1"),
                scaling_modifier=1.0, compute_cov3D_python=bool(z["compute_cov3D_python"]),
                scale_const=None if z["scale_const"] < 0 else float(z["scale_const"]), d_rot_as_res=bool(z["d_rot_as_res"]))


def near_plane_case(N, seed):
    """Points a few hundredths in front of both cameras' planes (h.w in [0.01, 0.1], |u| up to ~20): where the reference's
    plain division and the rasterizer's ``w + 1e-7`` part by far more than the rounding of either."""
    g = torch.Generator().manual_seed(seed)
    F1 = torch.tensor([[1.8, 0.0, 0.0, 0.0], [0.0, 2.2, 0.0, 0.0], [0.1, -0.05, 1.0001, 1.0], [0.02, 0.01, -0.01, 0.0]])
    F2 = torch.tensor([[1.79, 0.03, 0.01, 0.01], [-0.02, 2.2, 0.0, 0.0], [0.12, -0.04, 1.0001, 1.0], [0.05, 0.0, -0.01, 0.0]])
    xyz = torch.cat([torch.rand(N, 2, generator=g) * 0.8 - 0.4, 0.03 + 0.06 * torch.rand(N, 1, generator=g)], -1)
    d1 = 0.004 * torch.randn(N, 3, generator=g)
    d2 = 0.004 * torch.randn(N, 3, generator=g)
    return xyz, d1, d2, F1, F2


# ---- the torch-op form of render_flow over the drop-in rasterizer (GPU) ----------------------------------------------------
def render_flow_composed(pc, cam1, cam2, d_xyz1, d_xyz2, d_rotation1, d_scaling1, scaling_modifier=1.0,
                         compute_cov3D_python=False, scale_const=None, d_rot_as_res=True, colours_override=None):
    """What a user of the reference's render_flow runs over the drop-in ``GaussianRasterizer``: the colours and the glue in torch
    ops (above) on the raw parameters of ``pc``, then the rasterizer.  ``colours_override`` (N, 3) replaces the colours."""
    import math as m
    from riggs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    xyz = pc._xyz
    F2 = None if cam2 is None else cam2.full_proj_transform
    mask = torch.sigmoid(pc.feature[:, -1:]) if pc.with_motion_mask else None
    col = colours(xyz, d_xyz1, d_xyz2, cam1.full_proj_transform, F2, mask) if colours_override is None else colours_override
    glue = render_flow_glue(xyz, pc._scaling, pc._rotation, pc._opacity, bool(pc.use_isotropic_gs), d_xyz1, d_rotation1,
                            d_scaling1, scaling_modifier, compute_cov3D_python, scale_const, d_rot_as_res)
    settings = GaussianRasterizationSettings(
        image_height=int(cam1.image_height), image_width=int(cam1.image_width), tanfovx=m.tan(cam1.FoVx * 0.5),
        tanfovy=m.tan(cam1.FoVy * 0.5), bg=torch.zeros_like(col[0]), scale_modifier=scaling_modifier,
        viewmatrix=cam1.world_view_transform, projmatrix=cam1.full_proj_transform, sh_degree=0, campos=cam1.camera_center,
        prefiltered=False, debug=False)
    means2D = torch.zeros_like(xyz, requires_grad=True) + 0
    if means2D.requires_grad:
        means2D.retain_grad()
    image, radii, depth, alpha = GaussianRasterizer(raster_settings=settings)(
        means3D=glue["means3D"], means2D=means2D, shs=None, colors_precomp=col, opacities=glue["opacities"],
        scales=glue["scales"], rotations=glue["rotations"], cov3D_precomp=glue["cov3D_precomp"])
    return {"render": image, "depth": depth, "alpha": alpha, "viewspace_points": means2D, "visibility_filter": radii > 0,
            "radii": radii, "colours": col}
