"""-m gpu: a second colour set composited over a rendered frame's tile lists (csrc/recolor.hip, riggs_raster_recolor_forward /
_backward; riggs_amd.rasterizer.recolor_forward / recolor_backward; riggs_amd.render.recolor and render(keep_lists= / lists=)).

Scenes and seeds are those of test_gpu_raster.py's oracle parity cases (the oracle's contributor sets are known to agree with the
HIP forward's there).  Main render: SH colours over [0.1, 0.3, 0.7]; recolour: seeded (N, 3) colours in [-0.5, 1.5] over another
background; cotangent sign(rand - 0.5) / (3 H W).

Bounds: against the CPU oracle U.REL_TOL with the pixel share compare_forward_state grants the colour image (5e-6: no pixel at
these sizes) and _grads_close's 1e-5 of the elements; against the full HIP path 1e-5 / 1e-4 (image: the "fused vs general" bound)
and 2e-5 / 1e-4 (gradients: the bound between two atomic orders)."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import raster_ref as RR  # noqa: E402
from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import synth  # noqa: E402
from riggs_amd.gaussian_model import GaussianModel  # noqa: E402
from riggs_amd.loss import motion_mask_loss  # noqa: E402
from riggs_amd.rasterizer import (RasterArena, rasterize_backward, rasterize_forward, recolor_backward,  # noqa: E402
                                  recolor_forward, saved_views)
from riggs_amd.render import RenderPkg, recolor, render  # noqa: E402
from tests import gpu_util as U  # noqa: E402

BG1, BG2 = [0.1, 0.3, 0.7], [0.7, 0.2, 0.05]
PX_OUTLIER_FRAC = 5e-6  # compare_forward_state's allowance for the colour image
CASES = [
    (2000, 8, 1235, 128, 128, 0.03, dict()),
    (5000, 24, 7, 200, 333, 0.02, dict(azimuth_deg=90.0)),   # ragged image: partial tiles on both edges
    (30000, 24, 11, 96, 96, 0.05, dict()),                   # thousands of instances per tile, saturated pixels, most Gaussians untouched
    (3001, 24, 9, 160, 160, 0.25, dict(radius=1.2)),         # near-plane culls, huge splats, odd N
]
SEVEN = {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha", "bg_color"}


def _d(t):
    return None if t is None else t.cuda().contiguous()


def _bytes(t):
    return t.contiguous().view(torch.uint8).clone()


def _main_backward(s, act, gc):
    return rasterize_backward(s, _d(act["means3D"]), _d(act["shs"]), None, _d(act["opacities"]), _d(act["scales"]),
                              _d(act["rotations"]), None, None, None, gc, None, None)


@functools.lru_cache(maxsize=None)
def _case(i):
    """One main frame per case, shared by the tests (nothing below modifies it): the main frame's backward before the recolour,
    the recolour forward and backward, the main frame's backward after it, and the arenas' bytes before and after."""
    N, J, seed, H, W, scale, camkw = CASES[i]
    sc, act, cam = U.activated_scene(N, J, seed, H, W, scale=scale, **camkw)
    g = torch.Generator().manual_seed(seed + 100)
    col = torch.rand(N, 3, generator=g) * 2.0 - 0.5
    gc = torch.sign(torch.rand(3, H, W, generator=g) - 0.5) / (3 * H * W)
    gmain = torch.sign(torch.rand(3, H, W, generator=g) - 0.5) / (3 * H * W)
    color, radii, depth, alpha, s = U.hip_forward(act, cam, BG1)
    before = {k: _bytes(v) for k, v in saved_views(s).items() if isinstance(v, torch.Tensor)}
    arenas_before = [_bytes(s.geom), _bytes(s.img), _bytes(s.binning), _bytes(s.counters)]
    g_before = [None if t is None else t.clone() for t in _main_backward(s, act, _d(gmain))]
    image = recolor_forward(s, _d(col), torch.tensor(BG2, device="cuda"))
    grad = recolor_backward(s, _d(gc))
    torch.cuda.synchronize()
    after = {k: _bytes(v) for k, v in saved_views(s).items() if isinstance(v, torch.Tensor)}
    arenas_after = [_bytes(s.geom), _bytes(s.img), _bytes(s.binning), _bytes(s.counters)]
    g_after = _main_backward(s, act, _d(gmain))
    return dict(act=act, cam=cam, col=col, gc=gc, s=s, image=image, grad=grad, g_before=g_before, g_after=g_after, before=before,
                after=after, arenas_before=arenas_before, arenas_after=arenas_after, N=N, H=H, W=W)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_recolor_against_the_cpu_oracle(i):
    c = _case(i)
    out_o, so = U.oracle_forward(c["act"], c["cam"], BG2, colors=c["col"])
    go = RR.backward(so, c["gc"].numpy(), None, None)
    assert c["image"].shape == (3, c["H"], c["W"]) and c["grad"].shape == (c["N"], 3)
    U.assert_close(c["image"].cpu().numpy(), out_o["color"], "recolor image vs oracle", U.REL_TOL, PX_OUTLIER_FRAC)
    U.assert_close(c["grad"].cpu().numpy(), go["colors_precomp"].reshape(c["N"], 3), "recolor dL/dcolors vs oracle", U.REL_TOL, 1e-5)
    if i == 2:  # the case is there for the n_contrib bound and the sparse gradient: make sure it exercises them
        untouched = float((c["grad"].abs().sum(1) == 0).float().mean())
        assert 0.5 < untouched < 1.0, untouched
        v = saved_views(c["s"])
        rg = v["ranges"].long()
        assert int((rg[:, 1] - rg[:, 0]).max()) > 4 * 256  # several staging rounds
        T = (c["W"] // 16) * (c["H"] // 16)
        tile_len = (rg[:, 1] - rg[:, 0]).reshape(c["H"] // 16, c["W"] // 16).repeat_interleave(16, 0).repeat_interleave(16, 1)
        assert T == rg.shape[0] and bool((v["n_contrib"].long() < tile_len).any())  # pixels that stopped before their list's end


@pytest.mark.parametrize("i", range(len(CASES)))
def test_recolor_against_the_full_render_of_the_same_colours(i):
    c = _case(i)
    act = c["act"]
    color2, _, _, _, s2 = U.hip_forward(act, c["cam"], BG2, colors=c["col"])
    g2 = rasterize_backward(s2, _d(act["means3D"]), None, _d(c["col"]), _d(act["opacities"]), _d(act["scales"]),
                            _d(act["rotations"]), None, None, None, _d(c["gc"]), None, None)[3]
    U.assert_close(c["image"].cpu().numpy(), color2.cpu().numpy(), "recolor image vs full render", 1e-5, 1e-4)
    U.assert_close(c["grad"].cpu().numpy(), g2.cpu().numpy(), "recolor dL/dcolors vs full backward", 2e-5, 1e-4)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_recolor_leaves_the_main_frame_untouched(i):
    c = _case(i)
    for k in c["before"]:
        assert torch.equal(c["before"][k], c["after"][k]), "the recolour changed the frame's " + k
    for a, b, nm in zip(c["arenas_before"], c["arenas_after"], ("geometry arena", "image state", "binning arena", "counters")):
        assert torch.equal(a, b), "the " + nm + " changed"
    names = "means3D means2D sh colors opac scales rots cov dscaling".split()
    for a, b, nm in zip(c["g_after"], c["g_before"], names):
        if b is None:
            continue
        U.assert_close(a.cpu().numpy(), b.cpu().numpy(), "main dL/d%s after the recolour" % nm, 2e-5, 1e-4)


def test_recolor_of_an_empty_scene_is_the_background():
    cam = synth.look_at_camera(48, 48)
    st = U.settings_for(cam, BG1)
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    s = rasterize_forward(st, z(0, 3), z(0, 16, 3), None, z(0, 1), z(0, 3), z(0, 4), None)[4]
    bg2 = torch.tensor(BG2, device="cuda")
    image = recolor_forward(s, z(0, 3), bg2)
    assert torch.equal(image, bg2[:, None, None].expand(3, 48, 48))
    assert recolor_backward(s, torch.ones(3, 48, 48, device="cuda")).shape == (0, 3)


def test_recolor_of_a_scene_behind_the_camera_is_the_background():
    sc, act, cam = U.activated_scene(500, 8, 3, 48, 48)
    cam_far = synth.look_at_camera(48, 48, radius=4.0)
    act["means3D"] = act["means3D"] * 0 + cam_far.camera_center
    color, radii, depth, alpha, s = U.hip_forward(act, cam_far, BG1)
    assert int(radii.max()) == 0
    bg2 = torch.tensor(BG2, device="cuda")
    image = recolor_forward(s, torch.rand(500, 3).cuda(), bg2)
    assert torch.equal(image, bg2[:, None, None].expand(3, 48, 48))
    assert float(recolor_backward(s, torch.ones(3, 48, 48, device="cuda")).abs().max()) == 0.0


def test_recolor_over_tight_lists_equals_the_canonical_recolor():
    c = _case(0)
    act, cam = c["act"], c["cam"]
    st = U.settings_for(cam, BG1, debug=True)
    arena = RasterArena(tight_lists=True)
    s = rasterize_forward(st, _d(act["means3D"]), _d(act["shs"]), None, _d(act["opacities"]), _d(act["scales"]),
                          _d(act["rotations"]), None, arena=arena)[4]
    assert s.cfg.tight_lists == 1 and saved_views(s)["R"] < saved_views(c["s"])["R"]
    image = recolor_forward(s, _d(c["col"]), torch.tensor(BG2, device="cuda"))
    grad = recolor_backward(s, _d(c["gc"]))
    U.assert_close(image.cpu().numpy(), c["image"].cpu().numpy(), "tight-lists recolor image", U.REL_TOL)
    U.assert_close(grad.cpu().numpy(), c["grad"].cpu().numpy(), "tight-lists recolor dL/dcolors", U.REL_TOL)


def test_recolor_of_an_overflowed_frame_is_zero():
    c = _case(0)
    s = copy.copy(c["s"])
    s.counters = c["s"].counters.clone()
    s.counters[1] = 1  # (the flag alone: the lists are whole, nothing faults)
    image = recolor_forward(s, _d(c["col"]), torch.tensor(BG2, device="cuda"))
    grad = recolor_backward(s, _d(c["gc"]))
    assert float(image.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0
    assert float(c["image"].abs().max()) > 0.0  # (the shared frame's own counters are untouched)


def test_recolor_node_is_differentiable_in_the_colours_only():
    c = _case(0)
    col = _d(c["col"]).requires_grad_(True)
    bg2 = torch.tensor(BG2, device="cuda", requires_grad=True)
    image = recolor(c["s"], col, bg2)
    (image * _d(c["gc"])).sum().backward()
    assert torch.equal(image.detach(), c["image"])  # (the forward has no atomics: bitwise repeatable)
    U.assert_close(col.grad.cpu().numpy(), c["grad"].cpu().numpy(), "autograd dL/dcolors", 2e-5, 1e-4)
    assert bg2.grad is None


# ---- through render() ----------------------------------------------------------------------------------------------------
class Pipe:
    convert_SHs_python = False
    compute_cov3D_python = False
    debug = False


class PipeDebug(Pipe):
    debug = True


MOTION = dict(render_motion=True, detach_xyz=True, detach_rot=True, detach_scale=True, detach_opacity=True)


@functools.lru_cache(maxsize=None)
def _model():
    N, H, W = 6000, 160, 160
    sc = synth.make_scene(N, 24, 1240, scale=0.03)
    cam = synth.look_at_camera(H, W, fid=0.41).to("cuda")
    gm = GaussianModel.from_tensors(sc["xyz"], sc["features_dc"], sc["features_rest"], sc["scaling"], sc["rotation"], sc["opacity"])
    g = torch.Generator().manual_seed(2)
    gm.fea_dim, gm.with_motion_mask = 9, True
    gm.feature = torch.nn.Parameter(torch.randn(N, 9, generator=g).cuda())
    d = dict(gm=gm, cam=cam, N=N, H=H, W=W, bg=torch.tensor(BG1, device="cuda"),
             dx=(0.01 * torch.randn(N, 3, generator=g)).cuda(), dr=(0.01 * torch.randn(N, 4, generator=g)).cuda(),
             ds=torch.zeros(N, 3, device="cuda"),
             gimg=(torch.sign(torch.rand(3, H, W, generator=g) - 0.5) / (3 * H * W)).cuda(),
             gt=(torch.rand(1, H, W, generator=g) > 0.5).float().cuda(), ov=torch.rand(N, 3, generator=g).cuda())
    return d


def _zero_grads(m):
    for p in m["gm"].parameters() + [m["gm"].feature]:
        p.grad = None


def _main(m, arena, **kw):
    return render(m["cam"], m["gm"], Pipe, m["bg"], m["dx"], m["dr"], m["ds"], arena=arena, **kw)


def test_motion_render_over_the_main_frames_lists():
    m = _model()
    gm = m["gm"]
    arena = RasterArena()
    _main(m, arena)  # (the arena's first frame reads the instance count on the host; the frame under test is a later one)
    # the parent's way: the general path in an arena of its own
    _zero_grads(m)
    ref = render(m["cam"], gm, Pipe, m["bg"], m["dx"], m["dr"], m["ds"], **MOTION)
    motion_mask_loss(m["gt"], ref["render"][0]).backward()
    ref_image, ref_feature_grad = ref["render"].detach().clone(), gm.feature.grad[:, -1].clone()
    # main only
    _zero_grads(m)
    (_main(m, arena)["render"] * m["gimg"]).sum().backward()
    main_only = [p.grad.clone() for p in gm.parameters()]
    # main with kept lists + the motion render over them, one backward over both
    _zero_grads(m)
    main = _main(m, arena, keep_lists=True)
    assert isinstance(main, RenderPkg) and main.lists is not None and set(main.keys()) == SEVEN
    motion = render(m["cam"], gm, Pipe, m["bg"], m["dx"], m["dr"], m["ds"], lists=main.lists, **MOTION)
    assert set(motion.keys()) == SEVEN and set(ref.keys()) == SEVEN
    assert motion["radii"] is main["radii"] and torch.equal(motion["depth"], main["depth"]) and torch.equal(motion["alpha"], main["alpha"])
    assert torch.equal(motion["visibility_filter"], main["visibility_filter"])
    vp = motion["viewspace_points"]
    assert vp.shape == (m["N"], 3) and not vp.requires_grad and float(vp.abs().max()) == 0.0
    U.assert_close(motion["render"].detach().cpu().numpy(), ref_image.cpu().numpy(), "motion image: lists= vs its own render", 1e-5, 1e-4)
    loss = (main["render"] * m["gimg"]).sum() + motion_mask_loss(m["gt"], motion["render"][0])
    loss.backward()
    U.assert_close(gm.feature.grad[:, -1].cpu().numpy(), ref_feature_grad.cpu().numpy(), "dL/d(motion logit): lists= vs its own render",
                   2e-5, 1e-4)
    for p, want, nm in zip(gm.parameters(), main_only, "xyz f_dc f_rest opacity scaling rotation".split()):
        U.assert_close(p.grad.cpu().numpy(), want.cpu().numpy(), "dL/d%s: main + motion vs main only" % nm, 2e-5, 1e-4)
    assert main["viewspace_points"].grad is not None and vp.grad is None


def test_override_colour_over_the_main_frames_lists_and_the_general_path_keeps_lists_too():
    m = _model()
    gm = m["gm"]
    args = (m["cam"], gm, Pipe, m["bg"], m["dx"], m["dr"], m["ds"])
    ref = render(*args, override_color=m["ov"])["render"].detach()
    main = _main(m, RasterArena(), keep_lists=True)
    got = render(*args, override_color=m["ov"], lists=main.lists)
    assert set(got.keys()) == SEVEN
    U.assert_close(got["render"].detach().cpu().numpy(), ref.cpu().numpy(), "override_color: lists= vs its own render", 1e-5, 1e-4)
    # the general path (here: a per-Gaussian opacity residual) hands its lists on as well
    gen = render(*args, d_opacity=torch.zeros(m["N"], 1, device="cuda"), keep_lists=True)
    assert isinstance(gen, RenderPkg) and set(gen.keys()) == SEVEN and gen.lists.N == m["N"]
    got2 = render(*args, override_color=m["ov"], lists=gen.lists)["render"].detach()
    U.assert_close(got2.cpu().numpy(), ref.cpu().numpy(), "override_color over the general path's lists", 1e-5, 1e-4)
    # random_bg_color: a background drawn anew, composited by the recolour (alpha + final_T = 1 to 2e-5: test_gpu_raster.py)
    rnd = render(*args, override_color=m["ov"], lists=gen.lists, random_bg_color=True)
    assert not torch.equal(rnd["bg_color"], m["bg"])
    want = got2 + (1.0 - gen["alpha"].detach()) * (rnd["bg_color"] - m["bg"])[:, None, None]
    assert float((rnd["render"].detach() - want).abs().max()) <= 5e-5


def test_lists_of_a_frame_whose_arena_has_rendered_since_are_refused():
    m = _model()
    arena = RasterArena()
    rest = (m["gm"], Pipe, m["bg"], m["dx"], m["dr"], m["ds"])
    main = _main(m, arena, keep_lists=True)
    render(m["cam"], *rest, lists=main.lists, **MOTION)  # fine
    _main(m, arena)  # another frame through the same arena
    with pytest.raises(L.RiggsHipError):
        render(m["cam"], *rest, lists=main.lists, **MOTION)
    with pytest.raises(L.RiggsHipError):
        recolor_forward(main.lists, m["ov"], m["bg"])
    # pipe.debug: another camera's matrices are noticed
    main = _main(m, arena, keep_lists=True)
    other = synth.look_at_camera(m["H"], m["W"], azimuth_deg=40.0, fid=0.41).to("cuda")
    rest_debug = (m["gm"], PipeDebug) + rest[2:]
    with pytest.raises(ValueError):
        render(other, *rest_debug, lists=main.lists, **MOTION)
    render(m["cam"], *rest_debug, lists=main.lists, **MOTION)
