"""GPU: the editor's display step (riggs_amd.viewer, csrc/viewer.hip) against its restatement (tests/viewer_ref.py, checked on
the CPU against the reference by tests/test_viewer_cpu.py).

Tolerance of the base colour (depth2normal, the modes, the resize), per case: 4x what the reference's own torch ops deviate in
float32 on the CPU from their float64 run (``dev32`` of tests/golden/viewer_frames.npz), at least 1e-6 — the project's convention
(tests/test_gpu_metrics.py).  Coverage and painted colours: exact.  Projected integer coordinates: exact, on points asserted to
lie >= 1e-3 px from an integer before truncation.  What the HIP path showed is written to profiles/viewer_parity.json when
RIGGS_WRITE_PROFILES=1 is set (the committed record is made that way)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import viewer_ref as VR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = np.load(os.path.join(ROOT, "tests", "golden", "viewer_frames.npz"))
SHOWN = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_record():
    yield
    if SHOWN and os.environ.get("RIGGS_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "viewer_parity.json"), "w") as f:
            json.dump({"largest_deviation": max(v["dev"] for v in SHOWN.values()),
                       "largest_deviation_over_tolerance": max(v["dev"] / v["tolerance"] for v in SHOWN.values()),
                       "cases": SHOWN}, f, indent=1)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _out(case):
    return {k: _dev(v) for k, v in VR.make_out(case).items()}


def _show(name, got, want, dev32):
    dev, tol = float(np.abs(got - want).max()), VR.tolerance(dev32)
    SHOWN[name] = {"dev": dev, "dev32": float(dev32), "tolerance": tol}
    print(name, SHOWN[name])
    return dev, tol


# --------------------------------------------------------------------------- depth range
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 37, 53), (1, 130, 257)])
@pytest.mark.parametrize("kind", ["signed", "constant"])
def test_depth_range_is_bit_identical_to_torch(shape, kind):
    from riggs_amd import viewer as V
    g = torch.Generator().manual_seed(shape[1] * 1000 + shape[2])
    d = (torch.randn(shape, generator=g) * 3.0 if kind == "signed" else torch.full(shape, -2.75)).cuda()
    if kind == "signed" and d.numel() > 1:
        assert float(d.min()) < 0 < float(d.max())
    r = V.depth_range(d)
    assert r.shape == (2,) and torch.equal(r, torch.stack([d.min(), d.max()]))
    if d.numel() > 4:  # the extremes in the last element and in the first
        e = d.clone().reshape(-1)
        e[-1], e[0] = 99.5, -99.5
        assert V.depth_range(e.reshape(shape)).tolist() == [-99.5, 99.5]


# --------------------------------------------------------------------------- depth2normal, the modes, the resize
@pytest.mark.parametrize("name,shape,kind", VR.D2N_CASES, ids=[c[0] for c in VR.D2N_CASES])
def test_depth2normal(name, shape, kind):
    from riggs_amd import viewer as V
    d = VR.make_depth(shape, kind)
    got = V.depth2normal(_dev(d))
    assert got.shape == (3,) + shape and got.is_contiguous()
    dev, tol = _show("depth2normal_" + name, got.double().cpu().numpy(), FRAMES["normal_" + name], float(FRAMES["dev32_d2n_" + name]))
    assert dev <= tol
    assert torch.equal(V.depth2normal(_dev(d)[0]), got)                      # (H, W) and (1, H, W) alike
    f = 1.7 * shape[1]
    assert np.abs(V.depth2normal(_dev(d), focal=f).double().cpu().numpy() - VR.depth2normal(d, focal=f)).max() <= tol


@pytest.mark.parametrize("name,mode,case,size", VR.FRAME_CASES, ids=[c[0] for c in VR.FRAME_CASES])
def test_modes_and_resize(name, mode, case, size):
    from riggs_amd import viewer as V
    out = VR.make_out(case)
    dev_out = {k: _dev(v) for k, v in out.items()}
    got = V.display_frame(dev_out, mode, size)
    assert got.shape == size + (3,) and got.is_contiguous() and got.dtype is torch.float32
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    dev, tol = _show(name, got.double().cpu().numpy(), VR.display_frame(out, mode, size), float(FRAMES["dev32_" + name]))
    assert dev <= tol
    if size == out["depth"].shape[1:]:                                        # the identity: bit-identical to the clamped input
        if mode in ("render", "skinning"):
            want = dev_out[mode]
        elif mode == "alpha":
            want = dev_out["alpha"].repeat(3, 1, 1)
        elif mode == "depth":
            d = dev_out["depth"].repeat(3, 1, 1)
            want = (d - d.min()) / (d.max() - d.min() + 1e-20)
        else:
            want = (V.depth2normal(dev_out["depth"]) + 1) / 2
        assert torch.equal(got, want.permute(1, 2, 0).clamp(0, 1))
    buf = torch.full(size + (3,), -1.0, device="cuda")
    assert V.display_frame(dev_out, mode, size, out_buffer=buf) is buf and torch.equal(buf, got)


def test_override_and_the_skinning_fallback():
    from riggs_amd import viewer as V
    out = _out("bg_37x53")
    a = V.display_frame(out, "depth", (20, 31), override=out["skinning"])
    assert torch.equal(a, V.display_frame(out, "skinning", (20, 31)))
    del out["skinning"]
    assert torch.equal(V.display_frame(out, "skinning", (20, 31)), V.display_frame(out, "render", (20, 31)))
    with pytest.raises(ValueError):
        V.display_frame(out, "normals", (20, 31))


# --------------------------------------------------------------------------- coverage, pixel for pixel
WIN = (45, 70)  # (rows, columns): neither a multiple of the 16-pixel tile


def _random_table(n, seed, everywhere=True):
    """n primitives in paint order: overlapping segments (thickness 1, 2, 3), zero-length segments, discs with a colour radius
    above their alpha radius, squares, primitives wholly off screen, segments with one end at the coordinate clamp, invalid ones
    interleaved; ``everywhere=False``: every primitive touches the tile at (16..31, 16..31), so that tile's list overflows."""
    rng = np.random.default_rng(seed)
    H, W = WIN
    rows = []
    for i in range(n):
        rgb = np.float32(rng.random(3))
        ok = rng.random() > 0.12
        lo, hi = ((-6, max(H, W) + 6) if everywhere else (17, 30))
        a = rng.integers(lo, hi, 2)
        b = rng.integers(-6, max(H, W) + 6, 2)
        k = rng.integers(0, 10)
        if k < 4:
            rec = VR._record(VR.SEGMENT, a, b, int(rng.integers(1, 4)), int(rng.integers(1, 4)), rgb, ok)
        elif k == 4:
            rec = VR._record(VR.SEGMENT, a, a, int(rng.integers(1, 4)), int(rng.integers(1, 4)), rgb, ok)          # zero length
        elif k == 5:
            far = np.array([8192, -8192])[rng.integers(0, 2, 2)]
            rec = VR._record(VR.SEGMENT, a, far, int(rng.integers(1, 4)), 2, rgb, ok)                              # one end at the clamp
        elif k < 8:
            rec = VR._record(VR.DISC, a, a, 2 * int(rng.integers(0, 7)), 2 * int(rng.integers(0, 5)), rgb, ok)
        elif k == 8:
            r = rng.integers(0, 5, 2)
            rec = VR._record(VR.SQUARE, a - r, a + r, 0, 0, rgb, ok)
        else:
            off = np.array([W + 40, -30]) if everywhere else a                                                  # wholly off screen
            rec = VR._record(VR.DISC, off, off, 10, 8, rgb, ok)
        rows.append(rec)
    return np.array(rows, np.int64).reshape(-1, 12)


def _base():
    rng = np.random.default_rng(77)
    return np.float32(rng.random((3,) + WIN))


@pytest.mark.parametrize("everywhere", [True, False], ids=["spread", "one_tile"])
@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 1100])
def test_coverage_pixel_for_pixel(n, everywhere):
    from riggs_amd import viewer as V
    t = _random_table(n, 100 + n, everywhere)
    if n >= 64:
        assert (t[:, 10] == 0).any() and (t[:, 10] == 1).any() and len(set(t[:, 0])) == 3
    base = _base()
    table = _dev(t, torch.int32)
    for rule in (VR.BLEND_ALPHA, VR.BLEND_MASK):
        got = V._compose(0, _dev(base), WIN, [table], [rule]).double().cpu().numpy()
        want = VR.blend(np.moveaxis(np.float64(base), 0, -1), t, rule)
        assert np.array_equal(got != np.moveaxis(base, 0, -1), want != np.moveaxis(base, 0, -1))                 # the mask
        assert np.array_equal(got, want)                                                                       # and the colours
    if n == 1100 and not everywhere:
        assert int((t[:, 10] == 1).sum()) > 512            # every valid primitive touches one tile: its list overflows and continues


def test_groups_blend_one_after_another():
    from riggs_amd import viewer as V
    tabs = [_random_table(n, 7 + n) for n in (300, 5, 0, 70)]
    sq = _random_table(40, 3)
    sq = sq[sq[:, 0] == VR.SQUARE]
    base = _base()
    got = V.display_frame({"render": _dev(base)}, "render", WIN, overlays=[_dev(t, torch.int32).reshape(-1, 12) for t in tabs],
                          control_points=_dev(sq, torch.int32))
    want = np.moveaxis(np.float64(base), 0, -1)
    for t in tabs:
        want = VR.blend(want, t, VR.BLEND_ALPHA)
    want = VR.blend(want, sq, VR.BLEND_MASK)
    assert np.array_equal(got.double().cpu().numpy(), want)


# --------------------------------------------------------------------------- projection
def _camera(H, W, K=None, **kw):
    from riggs_amd import synth
    cam = synth.look_at_camera(H, W, **kw).to("cuda")
    return types.SimpleNamespace(**{**cam.__dict__, "K": K})


def _np(t):
    return t.detach().double().cpu().numpy()


def _same_table(got, want):
    got = got.cpu().numpy().astype(np.int64)
    assert got.shape == want.shape and np.array_equal(got[:, 10], want[:, 10]) and np.array_equal(got[:, 0], want[:, 0])
    ok = want[:, 10] == 1
    assert np.array_equal(got[ok][:, :10], want[ok][:, :10])
    assert not got[:, 11].any()


def test_invalid_and_far_points_are_marked_not_drawn():
    from riggs_amd import viewer as V
    cam = _camera(45, 70)
    M = _np(cam.full_proj_transform)
    inv = np.linalg.inv(_np(cam.world_view_transform))
    eye = inv[3, :3]

    def off_screen(y):  # far to the right of the camera, one unit in front of it
        return np.float32((np.array([5000.0, y, 1.0, 1.0]) @ inv)[:3])

    def to_mid_pixel(p):  # (its x is clamped; keep its y in the middle of a pixel: float32 sums of terms this large err by ~0.01 px)
        v = VR.project_editor(p, M, 45, 70)[0][0, 1]
        return abs(v - np.floor(v) - 0.5)
    far = min((off_screen(y) for y in np.linspace(0.05, 0.25, 41)), key=to_mid_pixel)
    assert to_mid_pixel(far) < 0.2
    pts = np.float32([[0.1, 0.05, 0.0], [0.3, -0.2, 0.1], 2.0 * eye, [np.nan, 0, 0], [0, np.inf, 0], far, [-0.2, 0.3, 0.2]])
    parents = np.array([-1, 0, 1, 1, 0, 0, 5])
    uv, ok = VR.project_editor(pts, M, 45, 70)
    assert ok.tolist() == [True, True, False, False, False, True, True] and VR.margin(uv, ok) >= 1e-3
    assert np.abs(uv[5]).max() > VR.COORD_MAX                                   # beyond the clamp
    colors = np.float32(np.random.default_rng(1).random((7, 3)))
    got = V.skeleton_overlay(cam, _dev(pts), _dev(parents), node_colors=_dev(colors))
    want = VR.skeleton_table(uv, ok, parents, colors)
    _same_table(got, want)
    assert want[:, 10].tolist() == [1, 0, 0, 0, 1, 1] + [1, 1, 0, 0, 0, 1, 1] and np.abs(want[4, 1:5]).max() == VR.COORD_MAX
    base = _base()
    frame = V.display_frame({"render": _dev(base)}, "render", (45, 70), overlays=[got])
    assert np.array_equal(frame.double().cpu().numpy(), VR.blend(np.moveaxis(np.float64(base), 0, -1), want, VR.BLEND_ALPHA))


def _posed(J, chain, seed):
    """d_nodes of a J-joint skeleton posed through SkeletonWarp.node_deformation."""
    from riggs_amd import synth
    from riggs_amd.skeleton import SkeletonWarp
    g = torch.Generator().manual_seed(seed)
    joints, parents = synth.make_skeleton(g, J, chain)
    sw = SkeletonWarp(joints=joints, parent_indices=parents, K=-1, hyper_dim=8, use_skinning_weight_mlp=False,
                      use_template_offsets=False).cuda()
    q = torch.tensor([1.0, 0, 0, 0]) + 0.15 * torch.randn(J, 4, generator=g)
    x = sw.nodes[:, :3].detach()
    d = sw.node_deformation(x, {"local_rotation": q.cuda(), "global_trans": (0.03 * torch.randn(3, generator=g)).cuda()})
    return sw, (x + d["d_xyz"]).contiguous(), parents


def _scene(seed, H, W):
    """The end-to-end scene of one seed and the least distance of any compared coordinate to an integer."""
    from riggs_amd import viewer as V
    cam = _camera(H, W, azimuth_deg=25.0, elevation_deg=10.0, radius=3.2)
    sw, d_nodes, parents = _posed(24, False, seed)
    _, ref_nodes, ref_parents = _posed(3, True, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    cloud = 0.5 * torch.randn(60, 3, generator=g)
    opacity = torch.rand(60, 1, generator=g)
    steps = [(cloud + 0.04 * k * torch.randn(60, 3, generator=g)).cuda() for k in range(7)]
    traj = V.TrajectoryOverlay(gs_num=8, samp_num=5, thickness=1)
    for s in steps:
        traj.push(s, opacity=opacity.cuda(), start=torch.tensor([3]))
    M = _np(cam.full_proj_transform)
    radius = int((H + W) / 2 * 0.005)
    kpt = 7
    uv, ok = VR.project_editor(_np(d_nodes), M, H, W)
    uvr, okr = VR.project_editor(_np(ref_nodes), M, H, W)
    ring = np.stack([_np(s) for s in steps])[-5:][:, traj.idx.cpu().numpy()]
    uvt, okt = VR.project_editor(ring.reshape(-1, 3), M, H, W)
    uvk, okk = VR.project_render_rig(_np(d_nodes), _np(cam.world_view_transform), cam.FoVx, cam.FoVy, H, W)
    every = ok.all() and okr.all() and okt.all() and okk.all()
    m = min(VR.margin(uv, ok), VR.margin(uvr, okr), VR.margin(uvt, okt), VR.margin(uvk, okk), VR.margin(uv[kpt:kpt + 1], ok[kpt:kpt + 1], (-radius, radius)))
    return types.SimpleNamespace(cam=cam, sw=sw, d_nodes=d_nodes, parents=parents, ref_nodes=ref_nodes, ref_parents=ref_parents, traj=traj,
                                 opacity=opacity, uv=uv, ok=ok, uvr=uvr, okr=okr, uvt=uvt.reshape(5, 8, 2), okt=okt.reshape(5, 8), uvk=uvk,
                                 okk=okk, kpt=kpt, radius=radius, margin=m if every else 0.0, H=H, W=W)


@pytest.fixture(scope="module")
def scene():
    """The first seed whose projected points all lie >= 1e-3 px from an integer: rounding must not decide a pixel."""
    for seed in range(4100, 4116):
        s = _scene(seed, 64, 80)
        if s.margin >= 1e-3:
            return s
    raise AssertionError("no seed keeps every projected point 1e-3 px away from an integer")


def test_end_to_end_overlays_and_frame(scene):
    from riggs_amd import viewer as V
    from riggs_amd.playback import get_geometric_color
    s = scene
    assert s.margin >= 1e-3
    assert bool((s.opacity[s.traj.idx.cpu(), 0] > 0.1).all()) and len(set(s.traj.idx.tolist())) == 8 and int(s.traj.idx[0]) == \
        int(torch.nonzero(s.opacity[:, 0] > 0.1)[3])
    assert s.traj.samples() == (5, 2)                                           # 7 pushes into 5 slots: the ring wrapped
    template = s.sw.nodes[:, :3].detach()
    skel = V.skeleton_overlay(s.cam, s.d_nodes, s.parents, template_nodes=template)
    ref = V.reference_skeleton_overlay(s.cam, s.ref_nodes, s.ref_parents)
    ctrl = V.control_point_overlay(s.cam, s.d_nodes[s.kpt], s.H, s.W)
    traj = s.traj.primitives(s.cam)
    want_skel = VR.skeleton_table(s.uv, s.ok, s.parents.numpy(), np.float32(_np(get_geometric_color(template))))
    want_ref = VR.skeleton_table(s.uvr, s.okr, s.ref_parents.numpy(), np.float32(_np(get_geometric_color(s.ref_nodes))),
                                 edge_color=VR.REFERENCE_EDGE_COLOR, discs_first=True, color_radius=4, alpha_radius=4)
    want_ctrl = VR.square_table(s.uv[s.kpt:s.kpt + 1], s.ok[s.kpt:s.kpt + 1], s.radius)
    want_traj = VR.polyline_table(s.uvt, s.okt, V.jet_colors(8))
    for got, want in ((skel, want_skel), (ref, want_ref), (ctrl, want_ctrl), (traj, want_traj)):
        _same_table(got, want)
    assert want_skel.shape == (47, 12) and want_ref.shape == (5, 12) and want_traj.shape == (32, 12) and want_ctrl.shape == (1, 12)
    inside = (want_skel[:, 1] >= 0) & (want_skel[:, 1] < s.W) & (want_skel[:, 2] >= 0) & (want_skel[:, 2] < s.H)
    assert inside.sum() >= 10                                                   # (not an empty picture)
    out = VR.make_out("bg_37x53")
    dev_out = {k: _dev(v) for k, v in out.items()}
    for mode in ("render", "depth"):
        got = V.display_frame(dev_out, mode, (s.H, s.W), overlays=[traj, skel, ref], control_points=ctrl).double().cpu().numpy()
        want = VR.display_frame(out, mode, (s.H, s.W), overlays=[want_traj, want_skel, want_ref], control_points=want_ctrl)
        plain = VR.display_frame(out, mode, (s.H, s.W))
        painted = (want != plain).any(-1)
        assert painted.sum() > 200 and np.array_equal(got[painted], want[painted])   # overlay pixels are exact ...
        assert np.abs(got - want).max() <= VR.tolerance(float(FRAMES["dev32_%s_64x80" % mode]))   # ... the rest to the resize tolerance


def test_draw_skeleton_on_image_and_pick_joint(scene):
    from riggs_amd import viewer as V
    s = scene
    rgba = np.float32(np.random.default_rng(9).random((4, s.H, s.W)))
    got = V.draw_skeleton_on_image(s.cam, s.d_nodes, s.parents, _dev(rgba), thickness=1)
    want = VR.draw_skeleton_on_image(s.uvk, s.okk, s.parents.numpy(), rgba, thickness=1)
    assert got.shape == (4, s.H, s.W) and np.array_equal(got.double().cpu().numpy(), want)
    assert (want[3] == 1).sum() > 100 and not np.array_equal(s.uvk, s.uv)
    for mouse in ((10.7, 20.2), (40, 33), (79.9, 63.9), (-5, 300)):
        want_idx = VR.pick_joint(s.uv, mouse)
        d = np.sort(np.sqrt(((s.uv - np.array([int(mouse[0]), int(mouse[1])])) ** 2).sum(-1)))
        assert d[1] - d[0] > 1e-3                                               # (no tie for rounding to decide)
        got_idx = V.pick_joint(s.cam, s.d_nodes, mouse)
        assert got_idx.is_cuda and got_idx.dtype is torch.int64 and int(got_idx) == want_idx


# --------------------------------------------------------------------------- no host synchronisation
def test_display_frame_does_not_synchronise(scene):
    from riggs_amd import viewer as V
    s = scene
    dev_out = _out("bg_37x53")
    template = s.sw.nodes[:, :3].detach()
    colors = V.get_geometric_color(template)
    parents = s.parents.to("cuda", torch.int32)
    ref_parents = s.ref_parents.to("cuda", torch.int32)
    buf = torch.empty(s.H, s.W, 3, device="cuda")
    kp = s.d_nodes[s.kpt]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s.traj.push(s.d_nodes.repeat(3, 1)[:60])
        over = [s.traj.primitives(s.cam), V.skeleton_overlay(s.cam, s.d_nodes, parents, node_colors=colors),
                V.reference_skeleton_overlay(s.cam, s.ref_nodes, ref_parents, node_colors=colors[:3])]
        ctrl = V.control_point_overlay(s.cam, kp, s.H, s.W)
        for mode in VR.MODES:
            V.display_frame(dev_out, mode, (s.H, s.W), overlays=over, control_points=ctrl, out_buffer=buf)
        V.depth2normal(dev_out["depth"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf).all())
