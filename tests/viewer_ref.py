"""NumPy restatement of the editor's display step (riggs_amd/viewer.py, csrc/viewer.hip): float64 for arithmetic, exact Python /
int64 integers for coverage.  The projection rules, depth2normal, the bilinear resize, the mode bases, the paint-order
rasteriser and the two blends, each as the reference writes it (interactive_GUI.py:97-247, :511-664, :1358-1368;
render_rig.py:40-94; utils/other_utils.py:78-97), with the coverage rule of include/riggs_hip.h standing in for OpenCV."""
import math

import numpy as np

PRIM_WORDS = 12
SEGMENT, DISC, SQUARE = 0, 1, 2
BLEND_ALPHA, BLEND_MASK = 0, 1
COORD_MAX = 8192
EDGE_COLOR = (68 / 255, 114 / 255, 196 / 255)
REFERENCE_EDGE_COLOR = (237 / 255, 125 / 255, 49 / 255)


# --------------------------------------------------------------------------- projection
def project_editor(points, full_proj, image_height, image_width):
    """(uv (n, 2) float64, valid (n,)): x is scaled by the HEIGHT, y by the width, as the reference has it."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        hom = np.concatenate([p, np.ones_like(p[:, :1])], -1) @ np.asarray(full_proj, np.float64)
        uv = hom[:, :2] / hom[:, 3:]
        uv = (uv + 1) / 2 * np.array([image_height, image_width], np.float64)
    return uv, (hom[:, 3] > 0) & np.isfinite(uv).all(-1)


def project_render_rig(points, world_view, fovx, fovy, image_height, image_width, K=None):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    V = np.asarray(world_view, np.float64)
    fy = image_height / (2 * math.tan(fovy * 0.5))
    fx = image_width / (2 * math.tan(fovx * 0.5))
    cx, cy = (float(K[0, 2]), float(K[1, 2])) if K is not None else (image_width / 2, image_height / 2)
    t = p @ V[:3, :3] + V[3, :3]
    with np.errstate(all="ignore"):
        uv = np.stack([fx * t[:, 0] / t[:, 2] + cx + 0.5, fy * t[:, 1] / t[:, 2] + cy + 0.5], -1)
    return uv, (t[:, 2] > 0) & np.isfinite(uv).all(-1)


def to_pixel(v):
    """astype(np.int32) / .int() — toward zero — then the clamp to +-COORD_MAX; 0 where not finite (such a primitive is invalid)."""
    v = np.asarray(v, np.float64)
    v = np.where(np.isfinite(v), v, 0.0)
    return np.trunc(np.clip(v, -COORD_MAX, COORD_MAX)).astype(np.int64)


def margin(uv, valid, offsets=(0.0,)):
    """The least distance of a valid coordinate (plus each offset) to an integer: what rounding would have to bridge to move a pixel."""
    v = np.asarray(uv, np.float64)[np.asarray(valid, bool)]
    v = v[(np.abs(v) < COORD_MAX - 1).all(-1)]
    return min((float(np.abs(v + o - np.round(v + o)).min()) if v.size else 1.0) for o in offsets)


def _rgb_bits(c):
    return np.asarray(c, np.float32).view(np.int32).astype(np.int64)


def _record(kind, a, b, ec, ea, rgb, ok):
    r = np.zeros(PRIM_WORDS, np.int64)
    r[0], r[1:3], r[3:5], r[5], r[6], r[7:10], r[10] = kind, a, b, ec, ea, _rgb_bits(rgb), int(ok)
    return r


def skeleton_table(uv, valid, parents, node_colors, thickness=2, edge_color=EDGE_COLOR, discs_first=False, color_radius=6, alpha_radius=4):
    px = to_pixel(uv)
    n = len(px)
    edges = [_record(SEGMENT, px[i], px[parents[i]], thickness, thickness, edge_color, valid[i] and valid[parents[i]]) for i in range(1, n)]
    discs = [_record(DISC, px[i], px[i], 2 * color_radius, 2 * alpha_radius, node_colors[i], valid[i]) for i in range(n)]
    return np.array((discs + edges) if discs_first else (edges + discs), np.int64).reshape(-1, PRIM_WORDS)


def square_table(uv, valid, radius, color=(1.0, 0.0, 0.0)):
    uv = np.asarray(uv, np.float64)
    return np.array([_record(SQUARE, to_pixel(uv[i] - radius), to_pixel(uv[i] + radius), 0, 0, color, valid[i]) for i in range(len(uv))],
                    np.int64).reshape(-1, PRIM_WORDS)


def polyline_table(uv, valid, colors, thickness=1):
    """uv (S, G, 2), oldest sample first: track after track."""
    S, G = uv.shape[:2]
    px = to_pixel(uv)
    return np.array([_record(SEGMENT, px[s, g], px[s + 1, g], thickness, thickness, colors[g], valid[s, g] and valid[s + 1, g])
                     for g in range(G) for s in range(S - 1)], np.int64).reshape(-1, PRIM_WORDS)


# --------------------------------------------------------------------------- coverage
def covered(rec, H, W, box=None):
    """(in the colour shape, in the alpha shape): two (H, W) bool masks of one primitive, in exact integers; over the pixel rows
    and columns ``box = (y_lo, y_hi, x_lo, x_hi)`` (exclusive ends) when given."""
    kind, x0, y0, x1, y1, ec, ea = (int(v) for v in rec[:7])
    ylo, yhi, xlo, xhi = (0, H, 0, W) if box is None else box
    y, x = np.mgrid[ylo:yhi, xlo:xhi].astype(np.int64)
    if kind == SQUARE:
        m = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
        return m, m
    ex, ey = x - x0, y - y0
    num, den = 4 * (ex * ex + ey * ey), np.ones_like(x)
    if kind == SEGMENT:
        dx, dy = x1 - x0, y1 - y0
        l2, t = dx * dx + dy * dy, ex * dx + ey * dy
        if l2 > 0:
            fx, fy = x - x1, y - y1
            c = ex * dy - ey * dx
            far, body = t >= l2, (t > 0) & (t < l2)
            num = np.where(far, 4 * (fx * fx + fy * fy), np.where(body, 4 * c * c, num))
            den = np.where(body, l2, den)
    return num <= ec * ec * den, num <= ea * ea * den


def bounding_box(rec, H, W):
    """The window's rows and columns that a primitive can reach (its end points grown by its larger extent), or None."""
    kind, x0, y0, x1, y1, ec, ea = (int(v) for v in rec[:7])
    grow = 0 if kind == SQUARE else (max(ec, ea) + 1) // 2
    ylo, yhi = max(min(y0, y1) - grow, 0), min(max(y0, y1) + grow + 1, H)
    xlo, xhi = max(min(x0, x1) - grow, 0), min(max(x0, x1) + grow + 1, W)
    return (ylo, yhi, xlo, xhi) if ylo < yhi and xlo < xhi else None


def paint(table, H, W, boxed=False):
    """The two layers of one overlay, painted in table order (the last writer wins): rgb (H, W, 3) float64, alpha (H, W).
    ``boxed``: each primitive is evaluated over its bounding box only (the same picture; what a scan converter would touch)."""
    rgb, a = np.zeros((H, W, 3)), np.zeros((H, W))
    for rec in np.asarray(table).reshape(-1, PRIM_WORDS):
        if rec[10] == 0:
            continue
        box = bounding_box(rec, H, W) if boxed else (0, H, 0, W)
        if box is None:
            continue
        in_c, in_a = covered(rec, H, W, box)
        rgb[box[0]:box[1], box[2]:box[3]][in_c] = rec[7:10].astype(np.int32).view(np.float32).astype(np.float64)
        a[box[0]:box[1], box[2]:box[3]][in_a] = 1.0
    return rgb, a


def blend(base, table, rule):
    rgb, a = paint(table, base.shape[0], base.shape[1])
    if rule == BLEND_ALPHA:   # :642, :645, :649
        return base * (1 - a[..., None]) + rgb * a[..., None]
    return base * (rgb.sum(-1, keepdims=True) == 0) + rgb  # :652-654


# --------------------------------------------------------------------------- base colour
def depth2normal(depth, focal=None, dtype=np.float64):
    d = np.asarray(depth, dtype).reshape(depth.shape[-2:])
    if focal is None:
        focal = d.shape[-1] / 2 / np.tan(np.pi / 6)
    p = np.pad(d, 1, mode="edge")
    half = dtype(0.5)
    gx = -half * p[1:-1, :-2] + half * p[1:-1, 2:]
    gy = -half * p[:-2, 1:-1] + half * p[2:, 1:-1]
    with np.errstate(all="ignore"):
        n = np.stack([gx, gy], -1) / (d[..., None] + dtype(1e-10)) * dtype(focal)
        n = np.concatenate([n, np.ones_like(n[..., :1])], -1)
        n = n / np.sqrt((n * n).sum(-1, keepdims=True))
    return np.moveaxis(n, -1, 0)


def resize_bilinear(img, H, W):
    """F.interpolate(mode="bilinear", align_corners=False) of (C, h, w) as ATen computes it: src = scale (dst + 0.5) - 0.5,
    negative -> 0; i1 = i0 + (i0 < in - 1); the weights 1 - lambda, lambda."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[-2:]

    def taps(n_in, n_out):
        src = np.maximum(n_in / n_out * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = src - i0
        return i0, i1, 1 - l1, l1
    y0, y1, hy0, hy1 = taps(h, H)
    x0, x1, wx0, wx1 = taps(w, W)
    top = wx0 * img[:, y0][:, :, x0] + wx1 * img[:, y0][:, :, x1]
    bot = wx0 * img[:, y1][:, :, x0] + wx1 * img[:, y1][:, :, x1]
    return hy0[:, None] * top + hy1[:, None] * bot


def base_image(out, mode, override=None, focal=None):
    """:521-529, :611-614 — the (3, h, w) image that is resized."""
    if override is not None:
        return np.asarray(override, np.float64)
    if mode in ("render", "skinning"):
        return np.asarray(out[mode] if mode in out else out["render"], np.float64)
    if mode == "normal_dep":
        return (depth2normal(np.asarray(out["depth"], np.float64), focal) + 1) / 2
    img = np.repeat(np.asarray(out[mode], np.float64).reshape((1,) + tuple(out[mode].shape[-2:])), 3, 0)
    if mode == "depth":
        img = (img - img.min()) / (img.max() - img.min() + 1e-20)
    return img


def display_frame(out, mode, size, overlays=(), control_points=None, override=None, focal=None):
    """(H, W, 3) float64."""
    img = resize_bilinear(base_image(out, mode, override, focal), size[0], size[1])
    frame = np.ascontiguousarray(np.clip(np.moveaxis(img, 0, -1), 0.0, 1.0))
    for t in overlays:
        frame = blend(frame, t, BLEND_ALPHA)
    if control_points is not None:
        frame = blend(frame, control_points, BLEND_MASK)
    return frame


def draw_skeleton_on_image(uv, valid, parents, rgba, thickness=1):
    """render_rig.py:71-92: (4, H, W) float64."""
    rgba = np.asarray(rgba, np.float64)
    H, W = rgba.shape[1:]
    n = len(uv)
    black = skeleton_table(uv, valid, parents, np.zeros((n, 3)), thickness, (0, 0, 0), color_radius=3, alpha_radius=3)
    rgb, a = paint(black, H, W)
    img = np.moveaxis(rgba[:3], 0, -1) * (1 - a[..., None])
    return np.concatenate([np.moveaxis(img, -1, 0), np.where(a > 0, 1.0, rgba[3])[None]], 0)


def pick_joint(uv, mouse_xy):
    m = np.array([int(mouse_xy[0]), int(mouse_xy[1])], np.float64)
    return int(np.argmin(np.sqrt(((np.asarray(uv, np.float64) - m) ** 2).sum(-1))))


# --------------------------------------------------------------------------- seeded cases (shared by the golden maker and the tests)
SEED = 20261
MODES = ("render", "depth", "alpha", "normal_dep", "skinning")
D2N_CASES = (("bg_37x53", (37, 53), "background"), ("bg_16x16", (16, 16), "background"), ("const_16x16", (16, 16), "constant"))
# (name, mode, source case, window): up, down and identity from 37 x 53 in every mode, and normal_dep of the two 16 x 16 maps
FRAME_CASES = tuple(("%s_%dx%d" % (m, H, W), m, "bg_37x53", (H, W)) for m in MODES for (H, W) in ((64, 80), (20, 31), (37, 53))) + \
    (("normal_dep_bg16_16x16", "normal_dep", "bg_16x16", (16, 16)), ("normal_dep_bg16_40x24", "normal_dep", "bg_16x16", (40, 24)),
     ("normal_dep_const16_24x20", "normal_dep", "const_16x16", (24, 20)))


def make_depth(shape, kind, seed=SEED):
    """float32 (1, h, w).  "background": positive depth inside an ellipse, a ZERO background next to it; "constant": 3 everywhere."""
    h, w = shape
    rng = np.random.default_rng(seed + 131 * h + w)
    if kind == "constant":
        return np.full((1, h, w), 3.0, np.float32)
    y, x = np.mgrid[0:h, 0:w]
    inside = ((y - 0.45 * h) / (0.38 * h)) ** 2 + ((x - 0.55 * w) / (0.36 * w)) ** 2 < 1
    d = 3.0 + 0.8 * np.sin(0.3 * x) * np.cos(0.23 * y) + 0.2 * rng.random((h, w))
    return np.float32(np.where(inside, d, 0.0))[None]


def make_out(case):
    """render()'s dict for a D2N case: render and skinning reach outside [0, 1] (the clamp), alpha above 1."""
    _, shape, kind = next(c for c in D2N_CASES if c[0] == case)
    h, w = shape
    rng = np.random.default_rng(SEED + 7 * h + 3 * w)
    depth = make_depth(shape, kind)
    return {"render": np.float32(rng.random((3, h, w)) * 1.4 - 0.2), "skinning": np.float32(rng.random((3, h, w)) * 1.2 - 0.1),
            "depth": depth, "alpha": np.float32((depth > 0) * (0.3 + 0.8 * rng.random((1, h, w))))}


def tolerance(dev32):
    """The project's convention (tests/test_gpu_metrics.py): 4x what the float32 torch-op form deviates from float64, at least 1e-6."""
    return max(4.0 * dev32, 1e-6)
