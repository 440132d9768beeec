"""GPU: the optical-flow term of a stage-1 iteration — the flow-colour kernels and the flow-loss kernels (csrc/flow.hip) through
the C ABI and through ``riggs_amd.render.render_flow`` / ``riggs_amd.loss.optical_flow_loss`` — against the fixtures recorded
from the reference and the float64 restatement of tests/flow_ref.py, with the bounds derived there."""
import glob
import math
import os

import pytest
import torch

from riggs_amd import _lib as L
from riggs_amd import synth
from riggs_amd.gaussian_model import GaussianModel
from riggs_amd.loss import landmark_interpolate, optical_flow_loss
from riggs_amd.rasterizer import RasterArena
from riggs_amd.render import flow_colors, render_flow
from tests import flow_ref as FR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN, "flow_*.npz")) if "loss_ref" not in p)
ATOMICS = 2e-5  # the rasterizer backward's float atomics, of the largest element (tests/test_gpu_torch_ext.py)
WORST = {}      # what -> worst err / bound seen so far


def _note(what, r):
    """Prints a measured err / bound ratio when it is a new worst (run with -s to read them)."""
    if float(r) > WORST.get(what, -1.0):
        WORST[what] = float(r)
        print("[flow] %s: %.3f" % (what, float(r)))


def _model(xyz, scaling, rotation, opacity, feature, mask, iso):
    P = lambda t: torch.nn.Parameter(t.detach().clone().float().cuda().contiguous())  # noqa: E731
    n = xyz.shape[0]
    gm = GaussianModel(3, fea_dim=feature.shape[1] - (1 if mask else 0), with_motion_mask=mask, use_isotropic_gs=iso)
    gm._xyz, gm._scaling, gm._rotation, gm._opacity, gm.feature = P(xyz), P(scaling), P(rotation), P(opacity), P(feature)
    gm._features_dc, gm._features_rest = P(torch.zeros(n, 1, 3)), P(torch.zeros(n, 15, 3))
    return gm


def _fixture(case):
    z = FR.load_fixture(os.path.join(GOLDEN, "flow_%s.npz" % case))
    gm = _model(z["xyz"], z["scaling"], z["rotation"], z["opacity"], z["feature"], bool(z["with_motion_mask"]), bool(z["isotropic"]))
    c = lambda t: t.cuda().contiguous()  # noqa: E731
    cam1 = synth.Camera(int(z["H"]), int(z["W"]), z["fovx"], z["fovy"], c(z["view1"]), c(z["proj1"]), c(z["campos1"]), torch.tensor([0.37]))
    cam2 = synth.Camera(int(z["H"]), int(z["W"]), z["fovx"], z["fovy"], c(z["view1"]), c(z["proj2"]), c(z["campos1"]),
                        torch.tensor([0.41])) if z["has_camera2"] else None
    return z, gm, cam1, cam2


# ---- colours through the C ABI ---------------------------------------------------------------------------------------------
TAIL = 96


def _tailed(t, fill):
    """A flat device buffer holding ``t`` followed by TAIL floats of ``fill``; returns (buffer, view of the payload)."""
    buf = torch.full((t.numel() + TAIL,), fill, dtype=torch.float32, device="cuda")
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf, buf[:t.numel()].view(t.shape)


def _colour_inputs(N, seed):
    g = torch.Generator().manual_seed(seed)
    cam1 = synth.look_at_camera(800, 800, fid=0.3)
    cam2 = synth.look_at_camera(800, 800, azimuth_deg=49.0, elevation_deg=18.0, radius=4.2, fid=0.5)
    xyz = 0.5 * torch.randn(N, 3, generator=g).clamp(-3, 3)
    d1, d2 = 0.05 * torch.randn(N, 3, generator=g), 0.05 * torch.randn(N, 3, generator=g)
    feature = torch.randn(N, 5, generator=g)
    cot = torch.randn(N, 3, generator=g)
    if N > 4:
        cot[1] = 0.0          # a row without any incoming gradient
        cot[2, :2] = 0.0      # ... and one with a mask gradient only
    return xyz, d1, d2, cam1.full_proj_transform, cam2.full_proj_transform, feature, cot


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 300000])
@pytest.mark.parametrize("null", ["none", "d1", "d2", "logit", "all"])
def test_colour_kernels_through_the_c_abi(N, null):
    lib = L.lib()
    xyz, d1, d2, F1, F2, feature, cot = _colour_inputs(N, 1000 + N)
    nan = float("nan")
    bx, vx = _tailed(xyz, nan)
    b1, v1 = _tailed(d1, nan)
    b2, v2 = _tailed(d2, nan)
    bf, vf = _tailed(feature, nan)
    bg, vg = _tailed(cot, nan)
    F1d, F2d = F1.cuda().contiguous(), F2.cuda().contiguous()
    use1, use2, usel = null not in ("d1", "all"), null not in ("d2", "all"), null not in ("logit", "all")
    if usel and N:  # only the last column may be read
        keep = vf[:, -1].clone()
        vf.fill_(nan)
        vf[:, -1] = keep
    logit_ptr = (bf.data_ptr() + 4 * (feature.shape[1] - 1)) if usel else None
    bc, vc = _tailed(torch.zeros(N, 3), 12345.0)
    st = L.stream_ptr()
    L.check(lib.riggs_flow_colors_forward(N, bx.data_ptr(), b1.data_ptr() if use1 else None, b2.data_ptr() if use2 else None,
                                          F1d.data_ptr(), F2d.data_ptr(), logit_ptr, feature.shape[1], bc.data_ptr(), st),
            "riggs_flow_colors_forward")
    o1, w1 = _tailed(torch.zeros(N, 3), 12345.0)
    o2, w2 = _tailed(torch.zeros(N, 3), 12345.0)
    ol, wl = _tailed(torch.zeros(N), 12345.0)
    if N == 0 or use1 or use2 or usel:
        L.check(lib.riggs_flow_colors_backward(N, bx.data_ptr(), b1.data_ptr() if use1 else None, b2.data_ptr() if use2 else None,
                                               F1d.data_ptr(), F2d.data_ptr(), logit_ptr, feature.shape[1], bg.data_ptr(),
                                               o1.data_ptr() if use1 else None, o2.data_ptr() if use2 else None,
                                               ol.data_ptr() if usel else None, st), "riggs_flow_colors_backward")
    torch.cuda.synchronize()
    for b in (bc, o1, o2, ol):
        assert bool((b[-TAIL:] == 12345.0).all()), "a kernel wrote behind its output"
    if N == 0:
        return
    a1, a2 = (d1 if use1 else 0.0), (d2 if use2 else 0.0)
    lg = feature[:, -1] if usel else None
    r, units = FR.colour_ratio(vc, xyz, a1, a2, F1, F2, lg)
    _note("colours err/bound", r)
    _note("colours err in eps*max(|u|,1)", units)
    assert r <= 1.0, (r, units)
    if not usel:
        assert bool((vc[:, 2] == 1.0).all())
    if use1 or use2 or usel:
        got = (w1 if use1 else None, w2 if use2 else None, wl if usel else None)
        ratios = FR.colour_grad_ratios(got, cot, xyz, a1, a2, F1, F2, lg)
        for k, rr in zip(("d_xyz1", "d_xyz2", "logit"), ratios):
            _note("colour gradient err/bound " + k, rr)
        assert max(ratios) <= 1.0, ratios
        if N > 4:  # exact zeros where the incoming gradient is exactly zero
            for w, use in ((w1, use1), (w2, use2)):
                assert not use or (float(w[1].abs().max()) == 0.0 and float(w[2].abs().max()) == 0.0)
            assert not usel or float(wl[1]) == 0.0
    if null == "all":  # nothing to compute: the call is refused, not a silent no-op
        assert lib.riggs_flow_colors_backward(N, bx.data_ptr(), None, None, F1d.data_ptr(), F2d.data_ptr(), None, 0,
                                              bg.data_ptr(), None, None, None, st) != 0


def test_colours_near_the_camera_plane_follow_the_plain_division():
    """h.w in [0.01, 0.1]: the bound rejects ``w + 1e-7`` there (tests/test_flow_cpu.py), the kernel passes it."""
    xyz, d1, d2, F1, F2 = FR.near_plane_case(4000, 5)

    class PC:
        with_motion_mask = False
        get_xyz = xyz.cuda()
    cam1 = synth.Camera(8, 8, 0.7, 0.7, torch.eye(4).cuda(), F1.cuda(), torch.zeros(3).cuda(), torch.tensor([0.0]))
    cam2 = synth.Camera(8, 8, 0.7, 0.7, torch.eye(4).cuda(), F2.cuda(), torch.zeros(3).cuda(), torch.tensor([0.0]))
    a1, a2 = d1.cuda().requires_grad_(True), d2.cuda().requires_grad_(True)
    col = flow_colors(PC, cam1, cam2, a1, a2)
    r, units = FR.colour_ratio(col, xyz, d1, d2, F1, F2)
    _note("colours err/bound (near plane)", r)
    assert r <= 1.0 and units > 0
    with pytest.raises(L.RiggsHipError):  # only the float 0.0 stands for an absent residual
        flow_colors(PC, cam1, cam2, 0.5, a2)
    g = torch.randn(4000, 3, generator=torch.Generator().manual_seed(6))
    g1, g2 = torch.autograd.grad((col * g.cuda()).sum(), [a1, a2])
    ratios = FR.colour_grad_ratios((g1, g2, None), g, xyz, d1, d2, F1, F2)
    _note("colour gradient err/bound (near plane)", max(ratios))
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("case", CASES)
def test_colours_and_gradients_match_the_reference_fixtures(case):
    z, gm, cam1, cam2 = _fixture(case)
    a1, a2 = z["d_xyz1"].cuda().requires_grad_(True), z["d_xyz2"].cuda().requires_grad_(True)
    col = flow_colors(gm, cam1, cam2, a1, a2)
    lg = z["feature"][:, -1] if z["with_motion_mask"] else None
    args = (z["xyz"], z["d_xyz1"], z["d_xyz2"], z["proj1"], z["proj2"], lg)
    assert FR.colour_ratio(col, *args)[0] <= 1.0                                   # the float64 restatement
    err = (col.detach().cpu().double() - z["colors_precomp"].double()).abs()       # the reference's own float32 result
    bound = FR.colour_bounds(*args)["colour"] + z["colour_ref_err"]
    assert bool((err <= bound).all()), float((err / bound).max())
    (col * z["cotangent"].cuda()).sum().backward()
    got = (a1.grad, a2.grad, gm.feature.grad[:, -1] if lg is not None else None)
    assert max(FR.colour_grad_ratios(got, z["cotangent"], *args)) <= 1.0
    b = FR.colour_bounds(*args, g=z["cotangent"])
    for name, t, want, e in (("d_xyz1", a1.grad, z["grad_d_xyz1"], 0), ("d_xyz2", a2.grad, z["grad_d_xyz2"], 1)):
        assert bool(((t.cpu().double() - want.double()).abs() <= b[name] + float(z["grad_ref_err"][e])).all()), name
    if lg is not None:
        assert float(gm.feature.grad[:, :-1].abs().max()) == 0.0
        assert bool(((gm.feature.grad[:, -1].cpu().double() - z["grad_feature"][:, -1].double()).abs()
                     <= b["logit"] + float(z["grad_ref_err"][2])).all())
    else:
        assert gm.feature.grad is None


# ---- render_flow against the composition ------------------------------------------------------------------------------------
def _grads_of(pkg, leaves, cot_img, cot_alpha):
    loss = (pkg["render"] * cot_img).sum() + (pkg["alpha"] * cot_alpha).sum()
    return torch.autograd.grad(loss, leaves, allow_unused=True)


@pytest.mark.parametrize("with_arena", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_render_flow_against_the_composition(case, with_arena):
    z, gm, cam1, cam2 = _fixture(case)
    kw = FR.fixture_glue_args(z, "cuda")
    a1, a2 = kw.pop("d_xyz1").requires_grad_(True), z["d_xyz2"].cuda().requires_grad_(True)
    arena = RasterArena() if with_arena else None
    pkg = render_flow(gm, cam1, cam2, a1, a2, arena=arena, **kw)
    if with_arena:
        # the second frame of an arena no longer reads the instance count, and may fold a pixel's sum in another order (the
        # arena's walk history, riggs_amd/rasterizer.py): the same image to rounding
        again = render_flow(gm, cam1, cam2, a1, a2, arena=arena, **kw)
        assert arena.last_R >= 0 and torch.equal(again["radii"], pkg["radii"])
        for k in ("render", "depth", "alpha"):
            assert float((again[k] - pkg[k]).detach().abs().max()) <= 1e-6 * max(1.0, float(pkg[k].detach().abs().max())), k
    assert set(pkg) == {"render", "depth", "alpha", "viewspace_points", "visibility_filter", "radii"}
    H, W, N = int(z["H"]), int(z["W"]), z["xyz"].shape[0]
    assert pkg["render"].shape == (3, H, W) and pkg["alpha"].shape == (1, H, W) and pkg["radii"].shape == (N,)
    assert torch.equal(pkg["visibility_filter"], pkg["radii"] > 0) and int(pkg["visibility_filter"].sum()) > N // 2
    own = flow_colors(gm, cam1, cam2, a1, a2).detach()
    same = FR.render_flow_composed(gm, cam1, cam2, a1, a2, colours_override=own, **kw)
    for k in ("radii", "depth", "alpha", "render"):
        assert torch.equal(pkg[k], same[k]), k
    # fed the float64 restatement's colours (rounded to float32): within the colour bound times the pixel's alpha
    lg = z["feature"][:, -1] if z["with_motion_mask"] else None
    c64 = FR.colours(z["xyz"].double(), z["d_xyz1"].double(), z["d_xyz2"].double(), z["proj1"].double(), z["proj2"].double(),
                     None if lg is None else torch.sigmoid(lg.double()[:, None]))
    ref = FR.render_flow_composed(gm, cam1, cam2, a1, a2, colours_override=c64.float().cuda(), **kw)
    for k in ("radii", "depth", "alpha"):
        assert torch.equal(pkg[k], ref[k]), k
    cb = float(FR.colour_bounds(z["xyz"], z["d_xyz1"], z["d_xyz2"], z["proj1"], z["proj2"], lg)["colour"].max())
    err, allow = (pkg["render"] - ref["render"]).detach().abs(), cb * pkg["alpha"].detach()
    live = allow > 0
    _note("image err / (colour bound x alpha)", float((err[live.expand_as(err)] / allow.expand_as(err)[live.expand_as(err)]).max()))
    assert bool((err <= allow).all())
    # gradients: the torch-op form end to end (its own colours), the rasterizer's atomics noise
    g = torch.Generator().manual_seed(9)
    cot_img, cot_alpha = torch.randn(3, H, W, generator=g).cuda(), torch.randn(1, H, W, generator=g).cuda()
    leaves = [a1, a2, gm._xyz, gm._scaling, gm._rotation, gm._opacity, gm.feature]
    mine = _grads_of(pkg, leaves + [pkg["viewspace_points"]], cot_img, cot_alpha)
    torch_form = FR.render_flow_composed(gm, cam1, cam2, a1, a2, **kw)
    theirs = _grads_of(torch_form, leaves + [torch_form["viewspace_points"]], cot_img, cot_alpha)
    for name, m, t in zip(("d_xyz1", "d_xyz2", "_xyz", "_scaling", "_rotation", "_opacity", "feature", "means2D"), mine, theirs):
        assert (m is None) == (t is None), name
        if m is not None:
            assert float((m - t).abs().max()) <= ATOMICS * float(t.abs().max()), name
    assert mine[1] is not None and float(mine[1].abs().max()) > 0


# ---- the loss ---------------------------------------------------------------------------------------------------------------
def _loss_inputs(seed, C, H, W, MC, dead=False):
    g = torch.Generator().manual_seed(seed)
    image, gt = torch.rand(C, H, W, generator=g), torch.rand(C, H, W, generator=g)
    motion = 0.2 * torch.randn(3, H, W, generator=g)
    alpha = torch.rand(1, H, W, generator=g) * 0.6 + 0.45
    flow = 8.0 * torch.randn(H, W, 2, generator=g)
    masks = (torch.rand(H, W, MC, generator=g) > 0.45).float()
    if dead:
        masks[..., :2] = 0.0
    return [image, gt, motion, alpha, flow, masks, 0.30, 0.55]


@pytest.mark.parametrize("H,W", [(1, 1), (17, 33), (800, 800), (1080, 1920)])
@pytest.mark.parametrize("MC", [2, 3, 4])
def test_loss_kernels_through_the_c_abi(H, W, MC):
    lib = L.lib()
    args = _loss_inputs(H + MC, 3, H, W, MC)
    if (H, W) == (1, 1):
        args[3][:] = 0.95
        args[5][:] = 1.0
    nan = float("nan")
    bufs = [_tailed(t, nan) for t in args[:6]]
    n_state = lib.riggs_flow_loss_state_floats(H, W)
    assert n_state >= H * W + 1
    state, _ = _tailed(torch.zeros(n_state), 12345.0)
    out = torch.full((1 + TAIL,), 12345.0, device="cuda")
    st = L.stream_ptr()
    L.check(lib.riggs_flow_loss_forward(3, H, W, MC, *[b[0].data_ptr() for b in bufs], None, None, args[6], args[7], state.data_ptr(),
                                        out.data_ptr(), st), "riggs_flow_loss_forward")
    grad, vgrad = _tailed(torch.zeros(3, H, W), 12345.0)
    one = torch.ones(1, device="cuda")
    L.check(lib.riggs_flow_loss_backward(H, W, bufs[2][0].data_ptr(), bufs[4][0].data_ptr(), state.data_ptr(), one.data_ptr(),
                                         grad.data_ptr(), st), "riggs_flow_loss_backward")
    torch.cuda.synchronize()
    for b in (state, out, grad):
        assert bool((b[-TAIL:] == 12345.0).all()), "a kernel wrote behind its output"
    r_loss, r_grad, share = FR.loss_ratios(out[0], vgrad, *args)
    _note("loss err/bound", r_loss)
    _note("loss gradient err/bound", r_grad)
    assert r_loss <= 1.0 and r_grad <= 1.0 and share <= 1e-3, (r_loss, r_grad, share)
    assert float(out[0]) > 0


@pytest.mark.parametrize("fid_as", ["tensor", "float", "mixed"])
def test_loss_through_the_python_surface(fid_as):
    args = _loss_inputs(21, 3, 60, 45, 3)
    dev = [t.cuda() if isinstance(t, torch.Tensor) else t for t in args]
    if fid_as != "float":
        dev[6] = torch.tensor([args[6]], device="cuda")
    if fid_as == "tensor":
        dev[7] = torch.tensor([args[7]], device="cuda")
    motion = dev[2].requires_grad_(True)
    image = dev[0].requires_grad_(True)  # (the loss detaches it, as the reference does)
    loss = optical_flow_loss(image, dev[1], motion, dev[3], dev[4], dev[5], dev[6], dev[7])
    assert loss.dim() == 0
    (3.0 * loss).backward()
    assert image.grad is None
    r_loss, r_grad, share = FR.loss_ratios(loss, motion.grad / 3.0, *args)
    assert r_loss <= 1.0 and r_grad <= 1.0 and share <= 1e-3
    # a flow file of another size: the reference's nearest-neighbour interpolate, in the wrapper
    small_f, small_m = dev[4][::2, ::3].contiguous(), dev[5][::2, ::3].contiguous()
    up = lambda t: torch.nn.functional.interpolate(t.permute(2, 0, 1)[None], (60, 45))[0].permute(1, 2, 0)  # noqa: E731
    a = optical_flow_loss(dev[0], dev[1], dev[2], dev[3], small_f, small_m, 0.3, 0.55)
    b = optical_flow_loss(dev[0], dev[1], dev[2], dev[3], up(small_f).contiguous(), up(small_m).contiguous(), 0.3, 0.55)
    assert torch.equal(a, b)
    with pytest.raises(L.RiggsHipError):
        optical_flow_loss(args[0], args[1], args[2], args[3], args[4], args[5], 0.3, 0.55)  # host tensors
    # a flow view at an odd float offset (the kernels read pairs): same bits as the aligned tensor
    odd = torch.empty(60 * 45 * 2 + 1, device="cuda")[1:].view(60, 45, 2)
    odd.copy_(dev[4])
    assert odd.data_ptr() % 8 == 4
    m2 = dev[2].detach().clone().requires_grad_(True)
    c = optical_flow_loss(dev[0], dev[1], m2, dev[3], odd, dev[5], 0.3, 0.55)
    c.backward()
    m3 = dev[2].detach().clone().requires_grad_(True)
    d_ = optical_flow_loss(dev[0], dev[1], m3, dev[3], dev[4], dev[5], 0.3, 0.55)
    d_.backward()
    assert torch.equal(c, d_) and torch.equal(m2.grad, m3.grad)
    assert L.lib().riggs_flow_loss_backward(60, 45, dev[2].data_ptr(), odd.data_ptr(), dev[2].data_ptr(), dev[2].data_ptr(),
                                            dev[2].data_ptr(), L.stream_ptr()) != 0  # refused before any launch


def test_all_dead_mask_gives_exact_zeros():
    args = _loss_inputs(31, 3, 33, 47, 3, dead=True)
    dev = [t.cuda() if isinstance(t, torch.Tensor) else t for t in args]
    motion = dev[2].requires_grad_(True)
    loss = optical_flow_loss(dev[0], dev[1], motion, dev[3], dev[4], dev[5], dev[6], dev[7])
    loss.backward()
    assert float(loss) == 0.0 and float(motion.grad.abs().max()) == 0.0


def test_landmark_interpolate_drives_lambda_optical():
    lm, st = [1e-1, 1e-1, 1e-3, 0], [0, 15_000, 25_000, 25_001]
    assert landmark_interpolate(lm, st, 0) == pytest.approx(0.1) and landmark_interpolate(lm, st, 20_000) == pytest.approx(0.01)
    assert landmark_interpolate(lm, st, 25_001) == 0


# ---- a scene for the whole term -----------------------------------------------------------------------------------------------
def _scene(N=6000, H=96, W=96, seed=3, hyper=8):
    """An opaque blob of one colour (alpha > 0.9 over a good part of the image; the image term is flat inside it) and two
    nearby cameras / times."""
    g = torch.Generator().manual_seed(seed)
    xyz = 0.35 * torch.randn(N, 3, generator=g).clamp(-2.5, 2.5)
    feature = torch.cat([0.02 * torch.randn(N, hyper, generator=g), 2.0 + torch.randn(N, 1, generator=g)], -1)
    gm = _model(xyz, math.log(0.05) + 0.2 * torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g),
                3.0 + 0.5 * torch.randn(N, 1, generator=g), feature, True, False)
    cam1 = synth.look_at_camera(H, W, fid=0.3).to("cuda")
    cam2 = synth.look_at_camera(H, W, azimuth_deg=48.0, elevation_deg=19.0, fid=0.6).to("cuda")
    return gm, cam1, cam2


def _true_motion(xyz, t):
    """The known motion: nothing moves at t = 0.3 (the first frame), a sheared translation grows from there."""
    return (t - 0.3) * (torch.tensor([0.30, 0.20, 0.0], device=xyz.device) + 0.3 * xyz * torch.tensor([0.0, 1.0, 0.5], device=xyz.device))


def _synthetic_flow(gm, cam1, cam2):
    """RAFT-like supervision made by projecting a known motion: the flow image of the true displacements, in pixels."""
    with torch.no_grad():
        x = gm.get_xyz
        pkg = render_flow(gm, cam1, cam2, _true_motion(x, 0.3), _true_motion(x, 0.6), 0.0, 0.0)
        H, W = pkg["render"].shape[1:]
        flow = pkg["render"][:2].permute(1, 2, 0) * torch.tensor([W, H], device="cuda") / 2
        masks = torch.ones(H, W, 3, device="cuda")
        return flow.contiguous(), masks, pkg["alpha"]


def _warp(gm, M=256, hyper=8, seed=11):
    from riggs_amd.control_nodes import ControlNodeWarp
    from riggs_amd.node_network import DeformNetwork
    torch.manual_seed(seed)
    net = DeformNetwork(is_blender=True, local_frame=False, W=64).cuda()
    cn = ControlNodeWarp(node_num=M, K=3, local_frame=False, d_rot_as_res=True, hyper_dim=hyper, network=net, is_blender=True).cuda()
    g = torch.Generator().manual_seed(seed)
    sel = torch.randperm(gm.get_xyz.shape[0], generator=g)[:M].cuda()
    with torch.no_grad():
        cn.nodes.copy_(torch.cat([gm.get_xyz.detach()[sel], gm.feature.detach()[sel, :hyper]], -1))
        cn._node_radius.fill_(math.log(0.2))
        cn._node_weight.zero_()
    return cn


class _Term:
    """The optical-flow term of an iteration on static inputs: deformation at t2, render_flow, the loss, backward."""

    def __init__(self, seed=5):
        self.gm, self.cam1, self.cam2 = _scene()
        self.cn = _warp(self.gm)
        N = self.gm.get_xyz.shape[0]
        g = torch.Generator().manual_seed(seed)
        self.flow, self.masks, _ = _synthetic_flow(self.gm, self.cam1, self.cam2)
        self.image, self.gt = torch.rand(3, 96, 96, generator=g).cuda(), torch.rand(3, 96, 96, generator=g).cuda()
        self.d1 = (0.02 * torch.randn(N, 3, generator=g)).cuda().requires_grad_(True)
        self.d2_extra = (0.02 * torch.randn(N, 3, generator=g)).cuda()
        self.fid1, self.fid2 = torch.tensor([0.3], device="cuda"), torch.tensor([0.6], device="cuda")
        self.arena = RasterArena()
        self.params = [p for p in self.cn.parameters()] + [self.gm.feature, self.d1]

    def new_inputs(self, seed):
        g = torch.Generator().manual_seed(seed)
        N = self.gm.get_xyz.shape[0]
        self.d2_extra.copy_((0.02 * torch.randn(N, 3, generator=g)).cuda())
        self.flow.copy_(self.flow + (0.5 * torch.randn(96, 96, 2, generator=g)).cuda())
        self.fid2.copy_(torch.tensor([0.45 + 0.3 * float(torch.rand(1, generator=g))]).cuda())

    def run(self):
        for p in self.params:
            p.grad = None
        gm = self.gm
        d2 = self.cn(gm.get_xyz.detach(), self.fid2.reshape(()), gm.feature, gm.motion_mask)["d_xyz"] + self.d2_extra
        d2.retain_grad()
        colours = flow_colors(gm, self.cam1, self.cam2, self.d1.detach(), d2.detach())
        pkg = render_flow(gm, self.cam1, self.cam2, self.d1, d2, 0.0, 0.0, arena=self.arena)
        pkg["render"].retain_grad()
        loss = optical_flow_loss(self.image, self.gt, pkg["render"], pkg["alpha"], self.flow, self.masks, self.fid1, self.fid2)
        loss.backward()
        net_grads = [p.grad for p in self.cn.network.parameters() if p.grad is not None]
        return dict(colours=colours, loss=loss.detach(), motion=pkg["render"].detach(), alpha=pkg["alpha"].detach(),
                    g_motion=pkg["render"].grad, g_d2=d2.grad, g_d1=self.d1.grad, g_net=net_grads)

    def warm(self, n=2):
        for _ in range(n):
            out = self.run()
            torch.cuda.current_stream().synchronize()
            self.arena.resolve()
        self.arena.top_up()
        return out


def _close(a, b, what):
    assert float((a - b).abs().max()) <= ATOMICS * float(b.abs().max()), what


def test_bitwise_repeatable_loss_and_backward_passes():
    args = [t.cuda() if isinstance(t, torch.Tensor) else t for t in _loss_inputs(41, 3, 800, 800, 3)]
    outs = []
    for _ in range(2):
        m = args[2].clone().requires_grad_(True)
        loss = optical_flow_loss(args[0], args[1], m, args[3], args[4], args[5], args[6], args[7])
        loss.backward()
        outs.append((loss.detach().clone(), m.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    xyz, d1, d2, F1, F2, feature, cot = _colour_inputs(300000, 77)
    gm = _model(xyz, torch.zeros(300000, 3), torch.ones(300000, 4), torch.zeros(300000, 1), feature, True, False)
    cam1 = synth.Camera(8, 8, 0.7, 0.7, torch.eye(4).cuda(), F1.cuda(), torch.zeros(3).cuda(), torch.tensor([0.0]))
    cam2 = synth.Camera(8, 8, 0.7, 0.7, torch.eye(4).cuda(), F2.cuda(), torch.zeros(3).cuda(), torch.tensor([0.0]))
    res = []
    for _ in range(2):
        a1, a2 = d1.cuda().requires_grad_(True), d2.cuda().requires_grad_(True)
        gm.feature.grad = None
        col = flow_colors(gm, cam1, cam2, a1, a2)
        (col * cot.cuda()).sum().backward()
        res.append((col.detach().clone(), a1.grad.clone(), a2.grad.clone(), gm.feature.grad.clone()))
    for u, v in zip(*res):
        assert torch.equal(u, v)


def test_whole_term_without_host_synchronisation():
    term = _Term()
    term.warm()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # positive control: the mode is honoured by this build
            torch.zeros(1, device="cuda").item()
        out = term.run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["loss"])) and float(out["loss"]) > 0 and len(out["g_net"]) > 0
    assert float((out["alpha"] > 0.9).float().mean()) > 0.05


def test_whole_term_captured_in_a_graph_replays_the_eager_run():
    term = _Term()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        term.warm()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            static = term.run()
        eager_arena = RasterArena()
        for rep in range(3):
            term.new_inputs(100 + rep)
            graph.replay()
            torch.cuda.synchronize()
            got = {k: ([g.clone() for g in v] if isinstance(v, list) else v.clone()) for k, v in static.items()}
            counters = term.arena.static_counters.tolist()
            assert counters[1] == 0, "the arena overflowed in a replay"
            # the colour and loss kernels: the same bits as an eager launch on the replay's inputs
            d2 = term.cn(term.gm.get_xyz.detach(), term.fid2.reshape(()), term.gm.feature, term.gm.motion_mask)["d_xyz"].detach() + term.d2_extra
            assert torch.equal(flow_colors(term.gm, term.cam1, term.cam2, term.d1.detach(), d2), got["colours"])
            m = got["motion"].clone().requires_grad_(True)
            loss = optical_flow_loss(term.image, term.gt, m, got["alpha"], term.flow, term.masks, term.fid1, term.fid2)
            loss.backward()
            assert torch.equal(loss.detach(), got["loss"]) and torch.equal(m.grad, got["g_motion"])
            # the whole term eagerly: what passes through the rasterizer agrees to its atomics' noise
            captured_arena, term.arena = term.arena, eager_arena  # (the graph owns its arena: an eager frame could regrow it)
            eager = term.run()
            term.arena = captured_arena
            torch.cuda.synchronize()
            assert torch.equal(eager["colours"], got["colours"])
            _close(eager["motion"], got["motion"], "motion")
            assert abs(float(eager["loss"]) - float(got["loss"])) <= ATOMICS * float(got["loss"])
            for k in ("g_d1", "g_d2"):
                _close(eager[k], got[k], k)
            assert len(eager["g_net"]) == len(got["g_net"]) > 0
            for a, b in zip(eager["g_net"], got["g_net"]):
                assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-12
    torch.cuda.current_stream().wait_stream(s)


def test_rows_without_a_colour_gradient_get_exact_zeros():
    """Two Gaussians that camera 1 culls, numerically on and well behind camera 2's plane (h.w ~ 0 and h.w < -1 there): exact
    zeros in both residual gradients, where the reference's autograd would form 0 * inf at h.w = 0; and the visible Gaussians'
    gradients are what they are when the two sit harmlessly in front of camera 2 instead."""
    z, gm, cam1, cam2 = _fixture("mask_aniso")
    F2 = z["proj2"].double()
    a1, a2 = z["d_xyz1"].cuda().clone(), z["d_xyz2"].cuda().clone()
    a2[0] = 0.0
    kw = FR.fixture_glue_args(z, "cuda")
    kw.pop("d_xyz1")

    def grads(xyz):
        gm._xyz.data = xyz.float().cuda()
        d1, d2 = a1.clone().requires_grad_(True), a2.clone().requires_grad_(True)
        pkg = render_flow(gm, cam1, cam2, d1, d2, **kw)
        g = torch.Generator().manual_seed(4)
        (pkg["render"] * torch.randn(3, int(z["H"]), int(z["W"]), generator=g).cuda()).sum().backward()
        hw = torch.cat([xyz[:2].double() + a2[:2].cpu().double(), torch.ones(2, 1, dtype=torch.float64)], -1) @ F2
        return d1.grad, d2.grad, pkg["radii"], hw[:, 3]
    n = F2[:3, 3] / F2[:3, 3].norm()                               # h.w = p . F2[:3, 3] + F2[3, 3]
    side = torch.linalg.cross(n, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))
    side = side / side.norm()
    on_plane = -F2[3, 3] / F2[:3, 3].norm() * n + 60.0 * side      # far off to the side: outside camera 1's image
    front, behind = z["xyz"].clone().double(), z["xyz"].clone().double()
    front[0], front[1] = on_plane + 3.0 * n, on_plane + 2.0 * n
    behind[0], behind[1] = on_plane, on_plane - 2.0 * n
    f1, f2, radii_f, hw_f = grads(front)
    b1, b2, radii_b, hw_b = grads(behind)
    assert float(hw_f.min()) > 1.0 and abs(float(hw_b[0])) < 1e-4 and float(hw_b[1]) < -1.0
    assert int(radii_f[:2].abs().sum()) == 0 and int(radii_b[:2].abs().sum()) == 0 and int((radii_b > 0).sum()) > 100
    for g_ in (f1, f2, b1, b2):
        assert bool(torch.isfinite(g_).all()) and float(g_[:2].abs().max()) == 0.0
    _close(b1[2:], f1[2:], "d_xyz1 of the other Gaussians")
    _close(b2[2:], f2[2:], "d_xyz2 of the other Gaussians")
    assert float(f2[2:].abs().max()) > 0


def _stage1_run(native, steps=20, lr=1e-2):
    """ControlNodeWarp + the native DeformNetwork, the image term and the flow term, ``steps`` Adam steps on the node network.
    The step size: the heads start at 1e-5 and only the time-dependent part of the network can lower the flow loss, so at the
    trainer's 1e-4 .. 1e-3 twenty steps move it by a fraction of a percent; at 1e-2 it falls by about two fifths."""
    from riggs_amd.graph import _Pipe
    from riggs_amd.loss import image_loss
    from riggs_amd.render import render
    gm, cam1, cam2 = _scene()
    cn = _warp(gm)
    flow, masks, alpha_true = _synthetic_flow(gm, cam1, cam2)
    assert float((alpha_true > 0.9).float().mean()) > 0.05
    with torch.no_grad():
        target = render(cam1, gm, _Pipe, torch.zeros(3, device="cuda"), _true_motion(gm.get_xyz, 0.3), 0.0, 0.0)["render"].clone()
    opt = torch.optim.Adam(list(cn.network.parameters()), lr=lr)
    t1, t2 = torch.tensor(0.3, device="cuda"), torch.tensor(0.6, device="cuda")
    lam = landmark_interpolate([1e-1, 1e-1, 1e-3, 0], [0, 15_000, 25_000, 25_001], 3000)
    # the flow term alone, through d_xyz2 alone, reaches the node network's time net
    x = gm.get_xyz.detach()
    d2 = cn(x, t2, gm.feature, gm.motion_mask)["d_xyz"]
    pkg2 = render_flow(gm, cam1, cam2, 0.0, d2, 0.0, 0.0)
    optical_flow_loss(target, target, pkg2["render"], pkg2["alpha"], flow, masks, 0.3, 0.6).backward()
    time_net_grad = float(cn.network.timenet[0].weight.grad.abs().max())
    flow_losses = []
    for it in range(steps):
        x = gm.get_xyz.detach()
        dv = cn(x, t1, gm.feature, gm.motion_mask, iteration=it)
        d_rot, d_scale = torch.zeros_like(dv["d_rotation"]), torch.zeros_like(dv["d_scaling"])
        pkg = render(cam1, gm, _Pipe, torch.zeros(3, device="cuda"), dv["d_xyz"], d_rot, d_scale)
        loss_img, _ = image_loss(pkg["render"], target, 0.2)
        d2 = cn(x, t2, gm.feature, gm.motion_mask, iteration=it)["d_xyz"]
        if native:
            pkg2 = render_flow(pc=gm, viewpoint_camera1=cam1, viewpoint_camera2=cam2, d_xyz1=dv["d_xyz"], d_xyz2=d2,
                               d_rotation1=d_rot, d_scaling1=d_scale, scale_const=None)
            lf = optical_flow_loss(pkg["render"], target, pkg2["render"], pkg2["alpha"], flow, masks, cam1.fid.cuda(), cam2.fid.cuda())
        else:
            pkg2 = FR.render_flow_composed(gm, cam1, cam2, dv["d_xyz"], d2, d_rot, d_scale)
            lf = FR.flow_loss(pkg["render"], target, pkg2["render"], pkg2["alpha"], flow, masks, cam1.fid.cuda(), cam2.fid.cuda())
        loss = loss_img + lam * lf
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(lf)) and bool(torch.isfinite(loss_img))
        opt.zero_grad()
        loss.backward()
        opt.step()
        flow_losses.append(float(lf.detach()))
    return flow_losses, time_net_grad


def test_short_stage1_run_with_the_flow_term():
    mine, tn = _stage1_run(True)
    theirs, tn_ref = _stage1_run(False)
    print("flow loss, native:", mine[0], "->", mine[-1], " torch-op form:", theirs[0], "->", theirs[-1])
    assert tn > 0 and tn_ref > 0
    assert mine[-1] < mine[0] and theirs[-1] < theirs[0]
    assert abs(mine[0] - theirs[0]) <= 1e-4 * theirs[0]
    assert abs((mine[0] - mine[-1]) - (theirs[0] - theirs[-1])) <= 0.25 * (theirs[0] - theirs[-1])
