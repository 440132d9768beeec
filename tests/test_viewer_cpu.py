"""CPU: the restatement of the editor's display step (tests/viewer_ref.py, which riggs_amd.viewer is pinned to) against what the
reference itself computed (tests/golden/viewer_*.npz, made by tests/golden/make_viewer_golden.py), against ``F.interpolate`` and
on hand-made paint-order cases; the header and the binding; the C entries' argument validation.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import viewer_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("riggs_viewer_depth_range", "riggs_viewer_depth2normal", "riggs_viewer_project_count", "riggs_viewer_project",
           "riggs_viewer_compose")


@pytest.fixture(scope="module")
def frames():
    return np.load(os.path.join(GOLDEN, "viewer_frames.npz"))


@pytest.fixture(scope="module")
def scene():
    return np.load(os.path.join(GOLDEN, "viewer_overlays.npz"))


def _rgb(table):
    return table[:, 7:10].astype(np.int32).view(np.float32)


# --------------------------------------------------------------------------- the goldens
@pytest.mark.parametrize("name,shape,kind", VR.D2N_CASES, ids=[c[0] for c in VR.D2N_CASES])
def test_depth2normal_equals_the_reference(frames, name, shape, kind):
    assert int(frames["seed"]) == VR.SEED
    d = VR.make_depth(shape, kind)
    if kind == "background":  # a zero background next to positive depth
        assert (d == 0).any() and (d > 0).any() and ((d[0, :, 1:] > 0) & (d[0, :, :-1] == 0)).any()
    got = VR.depth2normal(d)
    assert got.shape == (3,) + shape and np.abs(got - frames["normal_" + name]).max() <= 1e-12
    assert np.abs((got ** 2).sum(0) - 1).max() <= 1e-12
    assert 0 <= float(frames["dev32_d2n_" + name]) < 1e-5


def test_every_frame_case_has_its_recorded_float32_deviation(frames):
    for name, mode, case, size in VR.FRAME_CASES:
        assert 0 <= float(frames["dev32_" + name]) < 1e-4, name
    assert {m for _, m, _, _ in VR.FRAME_CASES} == set(VR.MODES)


def test_editor_skeleton_tables_equal_the_recorded_calls(scene):
    H, W = int(scene["H"]), int(scene["W"])
    assert H != W  # (x is scaled by the height: a square window would not tell)
    uv, ok = VR.project_editor(scene["d_nodes"], scene["full_proj"], H, W)
    assert ok.all() and VR.margin(uv, ok) >= 1e-3
    par, n = scene["parents"], 24
    t = VR.skeleton_table(uv, ok, par, scene["skel_disc_colors"], thickness=int(scene["skel_thickness"]))
    assert t.shape == (2 * n - 1, 12) and (t[:, 10] == 1).all()
    assert (t[:n - 1, 0] == VR.SEGMENT).all() and (t[n - 1:, 0] == VR.DISC).all()  # the bones first, then the discs
    assert np.array_equal(t[:n - 1, 1:5].reshape(-1, 2, 2), scene["skel_edges"])
    assert np.array_equal(t[n - 1:, 1:3], scene["skel_centers"]) and np.array_equal(t[n - 1:, 3:5], scene["skel_centers"])
    assert (t[:n - 1, 5] == 2).all() and (t[:n - 1, 6] == 2).all()
    assert int(scene["skel_color_radius"]) == 6 and int(scene["skel_alpha_radius"]) == 4
    assert (t[n - 1:, 5] == 12).all() and (t[n - 1:, 6] == 8).all()
    assert np.array_equal(_rgb(t[:n - 1]), np.float32(scene["skel_edge_colors"]))
    assert np.abs(scene["skel_edge_colors"] - np.array(VR.EDGE_COLOR)).max() == 0
    assert np.array_equal(_rgb(t[n - 1:]), np.float32(scene["skel_disc_colors"]))
    # the reference skeleton: discs of radius 4 / 4 BEFORE the bones
    uv, ok = VR.project_editor(scene["ref_nodes"], scene["full_proj"], H, W)
    assert VR.margin(uv, ok) >= 1e-3
    r = VR.skeleton_table(uv, ok, scene["ref_parents"], scene["ref_disc_colors"], thickness=int(scene["ref_thickness"]),
                          edge_color=VR.REFERENCE_EDGE_COLOR, discs_first=True, color_radius=4, alpha_radius=4)
    assert (r[:3, 0] == VR.DISC).all() and (r[3:, 0] == VR.SEGMENT).all()
    assert int(scene["ref_color_radius"]) == 4 and int(scene["ref_alpha_radius"]) == 4
    assert np.array_equal(r[:3, 1:3], scene["ref_centers"]) and np.array_equal(r[3:, 1:5].reshape(-1, 2, 2), scene["ref_edges"])
    assert np.abs(scene["ref_edge_colors"] - np.array(VR.REFERENCE_EDGE_COLOR)).max() == 0


def test_trajectory_and_control_point_tables_equal_the_recorded_calls(scene):
    from riggs_amd.viewer import jet_colors
    H, W = int(scene["H"]), int(scene["W"])
    G, S = scene["traj_pts"].shape[:2]
    ring = scene["traj_steps"][-S:, scene["traj_idx"]]       # the last S of the 7 pushes
    uv, ok = VR.project_editor(ring.reshape(-1, 3), scene["full_proj"], H, W)
    assert ok.all() and VR.margin(uv, ok) >= 1e-3
    t = VR.polyline_table(uv.reshape(S, G, 2), ok.reshape(S, G), jet_colors(G), thickness=int(scene["traj_thickness"]))
    assert t.shape == (G * (S - 1), 12)
    seg = t[:, 1:5].reshape(G, S - 1, 2, 2)
    assert np.array_equal(seg[:, :, 0], scene["traj_pts"][:, :-1]) and np.array_equal(seg[:, :, 1], scene["traj_pts"][:, 1:])
    assert np.array_equal(jet_colors(G), scene["traj_colors"])
    assert np.array_equal(_rgb(t).reshape(G, S - 1, 3)[:, 0], np.float32(scene["traj_colors"]))
    assert np.array_equal(jet_colors(512), np.load(os.path.join(GOLDEN, "viewer_jet512.npz"))["colors"])
    # the control point: trunc(uv - r) .. trunc(uv + r)
    k = int(scene["keypoint"])
    uv, ok = VR.project_editor(scene["d_nodes"][k:k + 1], scene["full_proj"], H, W)
    radius = int((H + W) / 2 * 0.005)
    assert VR.margin(uv, ok, (-radius, radius)) >= 1e-3
    sq = VR.square_table(uv, ok, radius)
    assert np.array_equal(sq[0, 1:3], scene["square_lt"]) and np.array_equal(sq[0, 3:5], scene["square_rb"])
    assert np.array_equal(_rgb(sq)[0], np.float32(scene["square_color"])) and sq[0, 0] == VR.SQUARE


@pytest.mark.parametrize("tag", ["rr", "rrK"])
def test_render_rig_tables_equal_the_recorded_calls(scene, tag):
    H, W = int(scene["H"]), int(scene["W"])
    uv, ok = VR.project_render_rig(scene["d_nodes"], scene["world_view"], float(scene["FoVx"]), float(scene["FoVy"]), H, W,
                                   scene["K"] if tag == "rrK" else None)
    assert ok.all() and VR.margin(uv, ok) >= 1e-3
    t = VR.skeleton_table(uv, ok, scene["parents"], np.zeros((24, 3)), thickness=int(scene[tag + "_thickness"]), edge_color=(0, 0, 0),
                          color_radius=int(scene[tag + "_color_radius"]), alpha_radius=int(scene[tag + "_alpha_radius"]))
    assert np.array_equal(t[:23, 1:5].reshape(-1, 2, 2), scene[tag + "_edges"]) and np.array_equal(t[23:, 1:3], scene[tag + "_centers"])
    assert (t[:23, 5] == 1).all() and (t[23:, 5] == 6).all() and (t[23:, 6] == 6).all()
    assert not scene[tag + "_edge_colors"].any() and not scene[tag + "_disc_colors"].any()
    assert not np.array_equal(scene["rr_centers"], scene["rrK_centers"])


def test_invalid_and_far_points():
    M = np.eye(4)
    M[2, 3], M[3, 3] = 1.0, 0.0           # w = z
    pts = np.array([[0.12, 0.21, 1.0], [0.1, 0.2, -1.0], [0.1, 0.2, 0.0], [np.nan, 0, 1.0], [1e7, -1e7, 1.0]])
    uv, ok = VR.project_editor(pts, M, 40, 60)
    assert ok.tolist() == [True, False, False, False, True]
    px = VR.to_pixel(uv)
    assert px[0].tolist() == [22, 36] and px[4].tolist() == [8192, -8192] and px[3].tolist() == [0, 0]
    assert VR.to_pixel(np.array([-0.7, 0.7, -3.2])).tolist() == [0, 0, -3]   # toward zero


# --------------------------------------------------------------------------- resize and modes
@pytest.mark.parametrize("size", [(64, 80), (20, 31), (37, 53), (1, 1), (74, 106), (111, 54)])
def test_resize_equals_interpolate(size):
    x = np.random.default_rng(5).random((3, 37, 53))
    want = torch.nn.functional.interpolate(torch.tensor(x)[None], size=size, mode="bilinear", align_corners=False)[0].numpy()
    got = VR.resize_bilinear(x, *size)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14
    if size == (37, 53):
        assert np.array_equal(got, x)


def test_mode_bases():
    out = VR.make_out("bg_37x53")
    f = VR.display_frame(out, "depth", (37, 53))
    assert f.shape == (37, 53, 3) and f.min() == 0.0 and abs(f.max() - 1.0) < 1e-12 and np.array_equal(f[..., 0], f[..., 2])
    const = VR.display_frame({"depth": np.full((1, 9, 7), 2.5, np.float32)}, "depth", (9, 7))
    assert not const.any()                                   # max - min = 0: 0 / 1e-20
    a = VR.display_frame(out, "alpha", (37, 53))
    assert np.array_equal(a[..., 1], np.clip(np.float64(out["alpha"][0]), 0, 1)) and out["alpha"].max() > 1
    r = VR.display_frame(out, "render", (37, 53))
    assert np.array_equal(r, np.clip(np.moveaxis(np.float64(out["render"]), 0, -1), 0, 1)) and out["render"].min() < 0
    s = VR.display_frame(out, "skinning", (37, 53))
    assert not np.array_equal(s, r)
    assert np.array_equal(VR.display_frame({"render": out["render"]}, "skinning", (37, 53)), r)
    n = VR.display_frame(out, "normal_dep", (37, 53))
    assert np.abs(n - np.moveaxis((VR.depth2normal(out["depth"]) + 1) / 2, 0, -1)).max() == 0
    o = VR.display_frame(out, "depth", (20, 31), override=out["skinning"])
    assert np.array_equal(o, VR.display_frame(out, "skinning", (20, 31)))


# --------------------------------------------------------------------------- paint order
def _disc(c, rc, ra, rgb, ok=True):
    return VR._record(VR.DISC, c, c, 2 * rc, 2 * ra, rgb, ok)


def _seg(a, b, t, rgb, ok=True):
    return VR._record(VR.SEGMENT, a, b, t, t, rgb, ok)


def test_the_colour_ring_between_radius_4_and_6_is_invisible():
    base = np.full((21, 21, 3), 0.25)
    out = VR.blend(base, np.array([_disc((10, 10), 6, 4, (1.0, 0.5, 0.0))]), VR.BLEND_ALPHA)
    y, x = np.mgrid[0:21, 0:21]
    d2 = (x - 10) ** 2 + (y - 10) ** 2
    assert (out[d2 <= 16] == np.array([1.0, 0.5, 0.0])).all() and (out[d2 > 16] == 0.25).all()
    assert int((d2 <= 16).sum()) == 49 and int(((d2 > 16) & (d2 <= 36)).sum()) == 64
    # ... away from the edges: a later bone's alpha over the ring shows the DISC's colour where the ring was painted last
    both = np.array([_seg((0, 15), (20, 15), 2, (0.0, 0.0, 1.0)), _disc((10, 10), 6, 4, (1.0, 0.5, 0.0))])
    out = VR.blend(base, both, VR.BLEND_ALPHA)
    assert (out[15, 10] == np.array([1.0, 0.5, 0.0])).all()   # inside the ring (d2 = 25), alpha from the bone, colour from the disc
    assert (out[15, 2] == np.array([0.0, 0.0, 1.0])).all() and (out[12, 2] == 0.25).all()
    out = VR.blend(base, both[::-1], VR.BLEND_ALPHA)          # the other order: the bone wins there
    assert (out[15, 10] == np.array([0.0, 0.0, 1.0])).all()


def test_segment_coverage_rule():
    H = W = 16
    one = VR.covered(_seg((2, 3), (12, 3), 1, (1, 1, 1)), H, W)[0]
    assert one.sum() == 11 and one[3, 2:13].all()                                   # dist^2 <= 1/4: the row itself
    two = VR.covered(_seg((2, 3), (12, 3), 2, (1, 1, 1)), H, W)[0]
    assert two[2:5, 2:13].all() and two[3, 1] and two[3, 13] and not two[2, 1] and two.sum() == 35   # round caps
    three = VR.covered(_seg((2, 3), (12, 3), 3, (1, 1, 1)), H, W)[0]
    assert three.sum() == 39 and np.array_equal(three & ~two, three ^ two)         # (3/2)^2 = 2.25 adds the offsets (+-1, +-1) ...
    assert three[2, 1] and three[4, 1] and three[2, 13] and three[4, 13]            # ... which lie beyond the two ends only
    zero = VR.covered(_seg((5, 5), (5, 5), 3, (1, 1, 1)), H, W)[0]
    disc = VR.covered(VR._record(VR.DISC, (5, 5), (5, 5), 3, 3, (1, 1, 1), True), H, W)[0]
    assert np.array_equal(zero, disc) and zero.sum() == 9                           # a zero-length segment is a disc of radius t / 2
    diag = VR.covered(_seg((0, 0), (15, 15), 1, (1, 1, 1)), H, W)[0]
    assert np.array_equal(diag, np.eye(16, dtype=bool))
    far = VR.covered(_seg((-8192, -8192), (8192, 8192), 1, (1, 1, 1)), H, W)[0]     # the largest operands: still exact
    assert np.array_equal(far, np.eye(16, dtype=bool))
    sq = VR.covered(VR._record(VR.SQUARE, (3, 4), (5, 9), 0, 0, (1, 0, 0), True), H, W)[0]
    assert sq.sum() == 3 * 6 and sq[4:10, 3:6].all()


def test_painting_over_bounding_boxes_gives_the_same_picture():
    rng = np.random.default_rng(3)
    recs = []
    for i in range(120):
        a, b = rng.integers(-20, 80, 2), rng.integers(-20, 80, 2)
        kind = int(rng.integers(0, 3))
        if kind == VR.SQUARE:
            b = a + rng.integers(0, 7, 2)
        recs.append(VR._record(kind, a, a if kind == VR.DISC else b, int(rng.integers(0, 9)), int(rng.integers(0, 9)), rng.random(3), i % 7 != 0))
    recs.append(_seg((30, 20), (8192, -8192), 3, (1, 1, 1)))
    full, boxed = VR.paint(np.array(recs), 45, 70), VR.paint(np.array(recs), 45, 70, boxed=True)
    assert np.array_equal(full[0], boxed[0]) and np.array_equal(full[1], boxed[1]) and 0 < full[1].mean() < 1


def test_the_control_point_mask_rule():
    base = np.full((12, 12, 3), 0.5)
    red = VR._record(VR.SQUARE, (2, 2), (4, 4), 0, 0, (1.0, 0.0, 0.0), True)
    out = VR.blend(base, np.array([red]), VR.BLEND_MASK)
    assert (out[2:5, 2:5] == np.array([1.0, 0.0, 0.0])).all() and (out[5:] == 0.5).all() and (out[:2] == 0.5).all()
    black = VR._record(VR.SQUARE, (6, 6), (8, 8), 0, 0, (0.0, 0.0, 0.0), True)
    assert (VR.blend(base, np.array([black]), VR.BLEND_MASK) == 0.5).all()          # sum(overlay) == 0 leaves the base
    hidden = VR._record(VR.SQUARE, (2, 2), (4, 4), 0, 0, (1.0, 0.0, 0.0), False)
    assert (VR.blend(base, np.array([hidden]), VR.BLEND_MASK) == 0.5).all()         # an invalid primitive is never drawn


# --------------------------------------------------------------------------- the C ABI
def test_header_declares_every_viewer_symbol_the_binding_has():
    from riggs_amd import _lib as L
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "riggs_hip.h")).read(), flags=re.S)
    # (the binding is read from the header; tests/test_capi_cpu.py has the compiler check every signature and layout)
    assert sorted(k for k in L.exported_symbols() if k.startswith("riggs_viewer_")) == sorted(SYMBOLS)
    for struct, cls in (("riggs_viewer_projection", L.ViewerProjection), ("riggs_viewer_frame", L.ViewerFrame)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
        names = [re.sub(r"\[.*?\]", "", n).strip(" *") for decl in body.split(";") if decl.strip()
                 for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?\s*", "", decl.strip(), count=1).split(",")]
        assert names == [f[0] for f in cls._fields_], struct
    assert "viewer.hip" in __import__("riggs_amd.build", fromlist=["SOURCES"]).SOURCES


def test_c_entries_reject_bad_arguments_without_a_gpu():
    from riggs_amd import _lib
    L = _lib.lib()
    P = 4096  # a non-NULL stand-in for a device pointer: never dereferenced on the host

    def rejected(rc, match):
        assert rc != 0 and match in L.riggs_last_error(), L.riggs_last_error()
    rejected(L.riggs_viewer_depth_range(0, P, P, P, None), b"empty")
    rejected(L.riggs_viewer_depth_range(10, None, P, P, None), b"NULL")
    rejected(L.riggs_viewer_depth2normal(0, 5, P, 1.0, P, None), b"shape")
    rejected(L.riggs_viewer_depth2normal(5, 5, P, 1.0, None, None), b"NULL")

    def proj(**kw):
        a = _lib.ViewerProjection()
        a.layout, a.n, a.points, a.matrix, a.table, a.parents = 0, 4, P, P, P, P
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert L.riggs_viewer_project_count(C.byref(proj())) == 7
    assert L.riggs_viewer_project_count(C.byref(proj(layout=1))) == 4
    assert L.riggs_viewer_project_count(C.byref(proj(layout=2, samples=5))) == 16
    assert L.riggs_viewer_project_count(C.byref(proj(layout=2, samples=1))) == 0
    assert L.riggs_viewer_project_count(C.byref(proj(layout=3))) < 0
    rejected(L.riggs_viewer_project(C.byref(proj(layout=3)), None), b"layout")
    rejected(L.riggs_viewer_project(C.byref(proj(rule=2)), None), b"rule")
    rejected(L.riggs_viewer_project(C.byref(proj(points=None)), None), b"NULL")
    rejected(L.riggs_viewer_project(C.byref(proj(parents=None)), None), b"parents")
    rejected(L.riggs_viewer_project(C.byref(proj(layout=2, samples=5, ring_capacity=4)), None), b"ring")
    rejected(L.riggs_viewer_project(C.byref(proj(segment_ext2=5000)), None), b"extent")

    def frame(**kw):
        f = _lib.ViewerFrame()
        f.mode, f.src_height, f.src_width, f.height, f.width, f.source, f.out = 0, 8, 8, 16, 16, P, P
        for k, v in kw.items():
            setattr(f, k, v)
        return f
    rejected(L.riggs_viewer_compose(C.byref(frame(mode=4)), None), b"mode")
    rejected(L.riggs_viewer_compose(C.byref(frame(width=0)), None), b"shape")
    rejected(L.riggs_viewer_compose(C.byref(frame(width=8193)), None), b"COORD_MAX")
    rejected(L.riggs_viewer_compose(C.byref(frame(out=None)), None), b"NULL")
    rejected(L.riggs_viewer_compose(C.byref(frame(mode=1)), None), b"range")
    rejected(L.riggs_viewer_compose(C.byref(frame(num_tables=9)), None), b"tables")
    f = frame(num_tables=1)
    f.counts[0] = 3
    rejected(L.riggs_viewer_compose(C.byref(f), None), b"table")
