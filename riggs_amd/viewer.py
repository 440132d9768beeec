"""The interactive editor's display step on the device: ``interactive_GUI.py::test_step`` (:497-664) from ``render()``'s dict to the
``(H, W, 3)`` buffer the window shows, including the overlays the reference draws with OpenCV on the host (skeleton :158-187,
reference skeleton :216-247, trajectories :127-155, control point :97-125), and ``render_rig.py``'s skeleton video frame
(:40-94), on the kernels of csrc/viewer.hip.  Inference only.

An overlay is a TABLE of primitives on the device — ``(P, 12)`` int32 records in paint order, the layout of
include/riggs_hip.h — made by ONE projection launch per builder; ``display_frame`` is one compose launch (plus the two-stage
depth range in ``depth`` mode) and never synchronises: the editor copies the finished buffer to the host once.

Two quirks of the reference are kept: the editor scales x by ``image_height`` and y by ``image_width`` (:143, :168, :228), and a
joint's colour disc has radius 6 while its alpha disc has radius 4 (:182-184), so only the inner disc shows.  Deviations: which
pixels a primitive covers follows the geometric rule stated in include/riggs_hip.h (OpenCV's scan conversion is not restated:
the package is no dependency of this library); primitives behind the camera or with a non-finite coordinate are not drawn; end
points are clamped to +-8192 pixels."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .playback import get_geometric_color


def _viewer(*names):
    """The header's RIGGS_VIEWER_* values of these names."""
    return [L.CONSTANTS["RIGGS_VIEWER_" + n] for n in names]


PRIM_WORDS, MAX_TABLES, RANGE_WORKSPACE_FLOATS = _viewer("PRIM_WORDS", "MAX_TABLES", "RANGE_WORKSPACE_FLOATS")
SEGMENT, DISC, SQUARE = _viewer("SEGMENT", "DISC", "SQUARE")
RULE_EDITOR, RULE_RENDER_RIG = _viewer("RULE_EDITOR", "RULE_RENDER_RIG")
LAYOUT_SKELETON, LAYOUT_SQUARES, LAYOUT_POLYLINES = _viewer("LAYOUT_SKELETON", "LAYOUT_SQUARES", "LAYOUT_POLYLINES")
BLEND_ALPHA, BLEND_MASK = _viewer("BLEND_ALPHA", "BLEND_MASK")
MODE_IMAGE, MODE_DEPTH, MODE_ALPHA, MODE_NORMAL = _viewer("MODE_IMAGE", "MODE_DEPTH", "MODE_ALPHA", "MODE_NORMAL")
MODES = {"render": MODE_IMAGE, "skinning": MODE_IMAGE, "depth": MODE_DEPTH, "alpha": MODE_ALPHA, "normal_dep": MODE_NORMAL}
EDGE_COLOR = (68 / 255, 114 / 255, 196 / 255)            # :173
REFERENCE_EDGE_COLOR = (237 / 255, 125 / 255, 49 / 255)  # :240

# matplotlib's published piecewise-linear definition of "jet" (x, y0, y1 per channel)
_JET = {"red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
        "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
        "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0))}


def jet_colors(gs_num=512):
    """:147, :152 — ``int32(cmap(i / max(1, gs_num - 1))[:3] * 255) / 255`` for i < gs_num with the 256-entry look-up table the
    package builds from ``_JET`` (entry k is the piecewise-linear ramp at k / 255; a value x reads entry ``int(x * 256)``, 255 at
    x = 1): a (gs_num, 3) float64 array.  No import of the package: tests/golden/viewer_jet512.npz pins it to the package's own."""
    n = 256
    lut = np.empty((n, 3))
    xind = np.linspace(0, n - 1, n)
    for c, name in enumerate(("red", "green", "blue")):
        d = np.array(_JET[name], dtype=float)
        x, y0, y1 = d[:, 0] * (n - 1), d[:, 1], d[:, 2]
        ind = np.searchsorted(x, xind)[1:-1]
        dist = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut[:, c] = np.clip(np.concatenate([[y1[0]], dist * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]]), 0.0, 1.0)
    xa = np.arange(gs_num) / max(1, float(gs_num - 1)) * n
    xa[xa == n] = n - 1
    idx = np.clip(xa.astype(int), 0, n - 1)
    return (lut[idx] * 255).astype(np.int32) / 255


# --------------------------------------------------------------------------- projection
def _matrix(camera, name, device):
    return L.require_cuda_f32("camera." + name, getattr(camera, name).to(device), (4, 4))


def _project(camera, points, layout, rule=RULE_EDITOR, parents=None, colors=None, rgb=(0, 0, 0, 0, 0, 0), samples=0, ring_head=0,
             ring_capacity=0, discs_first=False, segment_ext2=0, disc_color_ext2=0, disc_alpha_ext2=0, square_radius=0,
             want_table=True, want_uv=False):
    """One ``riggs_viewer_project`` launch: ``(table or None, uv or None)``."""
    points = L.require_cuda_f32("points", points.detach())
    dev = points.device
    a = L.ViewerProjection()
    a.layout, a.rule, a.samples, a.ring_head, a.ring_capacity, a.discs_first = layout, rule, samples, ring_head, ring_capacity, int(discs_first)
    a.n = points.shape[-2]
    a.segment_ext2, a.disc_color_ext2, a.disc_alpha_ext2, a.square_radius = segment_ext2, disc_color_ext2, disc_alpha_ext2, square_radius
    H, W = int(camera.image_height), int(camera.image_width)
    if rule == RULE_EDITOR:
        m = _matrix(camera, "full_proj_transform", dev)
        a.scale_x, a.scale_y = float(H), float(W)  # (x by the height, y by the width: the reference's order)
    else:  # render_rig.py:42-57
        m = _matrix(camera, "world_view_transform", dev)
        a.fx, a.fy = W / (2 * math.tan(camera.FoVx * 0.5)), H / (2 * math.tan(camera.FoVy * 0.5))
        K = getattr(camera, "K", None)
        a.cx, a.cy = (float(K[0, 2]), float(K[1, 2])) if K is not None else (W / 2, H / 2)
    keep = [points, m]
    a.points, a.matrix = points.data_ptr(), m.data_ptr()
    if parents is not None:
        parents = parents.to(dev, torch.int32).contiguous()
        if parents.numel() != a.n:
            raise L.RiggsHipError("parents has %d entries for %d points" % (parents.numel(), a.n))
        a.parents = parents.data_ptr()
        keep.append(parents)
    if colors is not None:
        colors = L.require_cuda_f32("colors", colors.detach().to(dev), (a.n, 3))
        a.colors = colors.data_ptr()
        keep.append(colors)
    a.rgb = (C.c_float * 6)(*[float(v) for v in rgb])
    lib = L.lib()
    P = int(lib.riggs_viewer_project_count(C.byref(a)))
    if P < 0:
        raise L.RiggsHipError("riggs_viewer_project_count: bad projection")
    table = torch.empty(P, PRIM_WORDS, dtype=torch.int32, device=dev) if want_table else None
    uv = torch.empty(a.n, 2, dtype=torch.float32, device=dev) if want_uv else None
    a.table, a.uv = L.ptr(table), L.ptr(uv)
    if P > 0:
        with torch.cuda.device(dev):
            L.check(lib.riggs_viewer_project(C.byref(a), L.stream_ptr()), "riggs_viewer_project")
    return table, uv


def _nodes(points, name):
    if points.dim() != 2 or points.shape[1] != 3:
        raise L.RiggsHipError("%s must be (n, 3), got %s" % (name, tuple(points.shape)))
    return points


@torch.no_grad()
def skeleton_overlay(camera, d_nodes, parents, node_colors=None, thickness=2, edge_color=EDGE_COLOR, template_nodes=None):
    """``update_skeleton_edges`` (:158-187): the bones joint -> parent in ``edge_color``, then a disc per joint — colour radius 6,
    alpha radius 4 — in ``node_colors`` (default: ``get_geometric_color(template_nodes)``, of ``d_nodes`` when no template is
    given).  The table ``(2 n - 1, 12)``."""
    d_nodes = _nodes(d_nodes, "d_nodes")
    if node_colors is None:
        node_colors = get_geometric_color((d_nodes if template_nodes is None else template_nodes[:, :3]).detach())
    return _project(camera, d_nodes, LAYOUT_SKELETON, parents=parents, colors=node_colors, rgb=tuple(edge_color) + (0, 0, 0),
                    segment_ext2=int(thickness), disc_color_ext2=12, disc_alpha_ext2=8)[0]


@torch.no_grad()
def reference_skeleton_overlay(camera, d_nodes, parents, node_colors=None, thickness=2, edge_color=REFERENCE_EDGE_COLOR):
    """``update_reference_skeleton`` (:216-247): the discs (radius 4 in both layers, ``get_geometric_color(d_nodes)``) are painted
    BEFORE the bones."""
    d_nodes = _nodes(d_nodes, "d_nodes")
    if node_colors is None:
        node_colors = get_geometric_color(d_nodes.detach())
    return _project(camera, d_nodes, LAYOUT_SKELETON, parents=parents, colors=node_colors, rgb=tuple(edge_color) + (0, 0, 0),
                    discs_first=True, segment_ext2=int(thickness), disc_color_ext2=8, disc_alpha_ext2=8)[0]


@torch.no_grad()
def control_point_overlay(camera, keypoints, H, W, color=(1.0, 0.0, 0.0)):
    """``update_control_point_overlay`` (:97-125): a filled red square of half side ``int((H + W) / 2 * 0.005)`` around each
    key point; give the table to ``display_frame(control_points=...)``, which blends it by the reference's mask rule."""
    keypoints = keypoints.reshape(-1, 3)
    return _project(camera, keypoints, LAYOUT_SQUARES, rgb=tuple(color) + (0, 0, 0), square_radius=int((H + W) / 2 * 0.005))[0]


class TrajectoryOverlay:
    """``update_trajectory_overlay`` (:127-155): the last ``samp_num`` positions of ``gs_num`` Gaussians picked by
    ``farthest_point_sample`` over those with opacity > 0.1, as polylines in the ``jet`` ramp.  The positions live in a ring on the
    device.  The first ``push`` picks the points (the boolean selection synchronises, once); later pushes and ``primitives`` do not."""

    def __init__(self, gs_num=512, samp_num=32, thickness=1):
        self.gs_num, self.samp_num, self.thickness = int(gs_num), int(samp_num), int(thickness)
        self.idx = self.ring = self.colors = None
        self.pushed = 0

    @torch.no_grad()
    def push(self, gs_xyz, opacity=None, start=None):
        """Append the current positions ``gs_xyz`` (N, 3).  ``opacity`` (N, 1): the activated opacities, read by the first push
        when their count matches (:131); ``start``: the sampler's first index (``None``: random, as the reference)."""
        from .fps import farthest_point_sample
        gs_xyz = L.require_cuda_f32("gs_xyz", gs_xyz.detach(), (None, 3))
        if self.idx is None:
            if opacity is not None and opacity.shape[0] == gs_xyz.shape[0]:
                mask = opacity.detach().reshape(gs_xyz.shape[0], -1)[:, 0] > .1
            else:
                mask = torch.ones_like(gs_xyz[:, 0], dtype=torch.bool)
            masked_idx = torch.arange(0, mask.shape[0], device=mask.device)[mask]
            self.idx = masked_idx[farthest_point_sample(gs_xyz[None, mask], self.gs_num, start=start)[0]]
            self.ring = torch.zeros(self.samp_num, self.gs_num, 3, dtype=torch.float32, device=gs_xyz.device)
            self.colors = torch.tensor(np.float32(jet_colors(self.gs_num)), device=gs_xyz.device)
        torch.index_select(gs_xyz, 0, self.idx, out=self.ring[self.pushed % self.samp_num])
        self.pushed += 1

    def samples(self):
        """(how many samples the ring holds, the slot of the oldest)"""
        S = min(self.pushed, self.samp_num)
        return S, (self.pushed - S) % self.samp_num

    @torch.no_grad()
    def primitives(self, camera):
        """The table ``(gs_num * (samples - 1), 12)``: track after track, oldest segment first."""
        if self.ring is None:
            raise L.RiggsHipError("TrajectoryOverlay.primitives before the first push")
        S, head = self.samples()
        return _project(camera, self.ring, LAYOUT_POLYLINES, colors=self.colors, samples=S, ring_head=head, ring_capacity=self.samp_num,
                        segment_ext2=self.thickness)[0]


@torch.no_grad()
def pick_joint(camera, d_nodes, mouse_xy):
    """:1358-1368: the joint whose projection (the editor rule, before truncation) is nearest to the integer mouse position, as a
    0-d int64 tensor on the device."""
    uv = _project(camera, _nodes(d_nodes, "d_nodes"), LAYOUT_SQUARES, want_table=False, want_uv=True)[1]
    mouse = torch.tensor([[int(mouse_xy[0]), int(mouse_xy[1])]], device=uv.device)
    return (uv - mouse).norm(dim=-1).argmin()


# --------------------------------------------------------------------------- frames
@torch.no_grad()
def depth_range(depth):
    """``(2,)`` = [min, max] of a depth map on the device: bit-identical to ``torch.min`` / ``torch.max``, without their two
    reductions' launches and with no atomics."""
    depth = L.require_cuda_f32("depth", depth.detach())
    ws = torch.empty(RANGE_WORKSPACE_FLOATS + 2, dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        L.check(L.lib().riggs_viewer_depth_range(depth.numel(), depth.data_ptr(), ws.data_ptr(), ws[RANGE_WORKSPACE_FLOATS:].data_ptr(),
                                                 L.stream_ptr()), "riggs_viewer_depth_range")
    return ws[RANGE_WORKSPACE_FLOATS:]


def _depth_hw(depth):
    if depth.dim() == 3:
        depth = depth.squeeze()
    if depth.dim() < 2:  # (a map of one row or one column squeezes further; keep it a map)
        depth = depth.reshape(1, -1) if depth.dim() == 1 else depth.reshape(1, 1)
    if depth.dim() != 2:
        raise L.RiggsHipError("depth must be (h, w) or (1, h, w), got %s" % (tuple(depth.shape),))
    return L.require_cuda_f32("depth", depth.detach())


def _focal(w, focal):
    return float(w / 2 / np.tan(np.pi / 6)) if focal is None else float(focal)


@torch.no_grad()
def depth2normal(depth, focal=None):
    """``utils/other_utils.py::depth2normal`` (:78-97): ``(3, H, W)`` unit normals from a depth map ``(H, W)`` or ``(1, H, W)``."""
    d = _depth_hw(depth)
    h, w = d.shape
    out = torch.empty(3, h, w, dtype=torch.float32, device=d.device)
    with torch.cuda.device(d.device):
        L.check(L.lib().riggs_viewer_depth2normal(h, w, d.data_ptr(), _focal(w, focal), out.data_ptr(), L.stream_ptr()),
                "riggs_viewer_depth2normal")
    return out


def _compose(mode, source, size, tables, rules, rng=None, focal=None, out_buffer=None):
    h, w = source.shape[-2:]
    H, W = int(size[0]), int(size[1])
    dev = source.device
    if out_buffer is None:
        out_buffer = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    elif tuple(out_buffer.shape) != (H, W, 3) or out_buffer.dtype is not torch.float32 or not out_buffer.is_contiguous() or out_buffer.device != dev:
        raise L.RiggsHipError("out_buffer must be a contiguous float32 (%d, %d, 3) tensor on %s" % (H, W, dev))
    if len(tables) > MAX_TABLES:
        raise L.RiggsHipError("at most %d overlay tables per frame" % MAX_TABLES)
    f = L.ViewerFrame()
    f.mode, f.src_height, f.src_width, f.height, f.width, f.num_tables = mode, h, w, H, W, len(tables)
    f.focal = _focal(w, focal)
    f.scale_h, f.scale_w = h / H, w / W
    f.source, f.range, f.out = source.data_ptr(), L.ptr(rng), out_buffer.data_ptr()
    for g, (t, r) in enumerate(zip(tables, rules)):
        if t.dtype is not torch.int32 or t.dim() != 2 or t.shape[1] != PRIM_WORDS or not t.is_contiguous() or t.device != dev:
            raise L.RiggsHipError("an overlay must be a contiguous int32 (P, %d) table on %s" % (PRIM_WORDS, dev))
        f.tables[g], f.counts[g], f.rules[g] = (t.data_ptr() if t.shape[0] else None), t.shape[0], r
    with torch.cuda.device(dev):
        L.check(L.lib().riggs_viewer_compose(C.byref(f), L.stream_ptr()), "riggs_viewer_compose")
    return out_buffer


@torch.no_grad()
def display_frame(out, mode, size, overlays=(), control_points=None, override=None, out_buffer=None, focal=None):
    """:511-664 — the frame the editor's window shows, ``(H, W, 3)`` float32 on the device (written into ``out_buffer`` if given).

    ``out``: ``render()``'s dict (``render``, ``depth``, ``alpha``; ``skinning`` if the caller rendered the skinning colours —
    otherwise that mode shows ``render``, as the reference's ``out["skinning"] = out["render"]``).  ``mode``: ``render``,
    ``depth`` (normalised by the frame's min and max), ``alpha``, ``normal_dep`` (``(depth2normal(depth) + 1) / 2``),
    ``skinning``.  ``override``: a ``(3, h, w)`` image shown instead of ``out[mode]``.  The base is resized to ``size = (H, W)``
    as ``F.interpolate(mode="bilinear", align_corners=False)`` and clamped to [0, 1]; then the ``overlays`` (tables of the
    builders above) are blended one after another in the given order — the reference's is trajectories, skeleton, reference
    skeleton (:641-649) — and ``control_points`` (a ``control_point_overlay`` table) last, by its mask rule (:651-654).
    Launches: the depth range (``depth`` mode only) and one compose.  No host synchronisation."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))
    m, rng = MODES[mode], None
    if override is not None:
        m, source = 0, override
    elif m == 0:
        source = out[mode] if mode in out else out["render"]
    else:
        source = out["alpha" if mode == "alpha" else "depth"]
    if m == 0:
        if source.dim() != 3 or source.shape[0] != 3:
            raise L.RiggsHipError("the image must be (3, h, w), got %s" % (tuple(source.shape),))
        source = L.require_cuda_f32("image", source.detach())
    else:
        source = _depth_hw(source)
        if m == 1:
            rng = depth_range(source)
    tables = list(overlays) + ([control_points] if control_points is not None else [])
    rules = [BLEND_ALPHA] * len(overlays) + ([BLEND_MASK] if control_points is not None else [])
    return _compose(m, source, size, tables, rules, rng=rng, focal=focal, out_buffer=out_buffer)


@torch.no_grad()
def draw_skeleton_on_image(camera, nodes, parents, rgba_image, thickness=1):
    """``project_nodes_to_2d_withnodes`` (render_rig.py:40-94) without the file write: black bones and black discs of radius 3
    painted into the colour channels of ``rgba_image`` (4, H, W) and ones into its alpha channel, with the ``render_rig``
    projection rule; ``(4, H, W)``.  (The channels pass through the display path's clamp to [0, 1].)"""
    if rgba_image.dim() != 3 or rgba_image.shape[0] != 4:
        raise L.RiggsHipError("rgba_image must be (4, H, W), got %s" % (tuple(rgba_image.shape),))
    img = L.require_cuda_f32("rgba_image", rgba_image.detach())
    H, W = img.shape[1:]
    black = _project(camera, _nodes(nodes, "nodes"), LAYOUT_SKELETON, rule=RULE_RENDER_RIG, parents=parents, segment_ext2=int(thickness),
                     disc_color_ext2=6, disc_alpha_ext2=6)[0]
    white = black.clone()
    white[:, 7:10] = 0x3f800000  # (the bits of 1.0f)
    rgb = _compose(MODE_IMAGE, img[:3], (H, W), [black], [BLEND_ALPHA])
    a = _compose(MODE_ALPHA, img[3], (H, W), [white], [BLEND_ALPHA])
    return torch.cat([rgb.permute(2, 0, 1), a.permute(2, 0, 1)[:1]], dim=0)
