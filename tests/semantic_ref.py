"""NumPy restatement of the nodes' semantic labels (csrc/semantic.hip; the reference's train_rig.py:177-190, 215-216, 227 over
utils/other_utils.py:101-127), and the cameras and scenes tests/test_gpu_semantic.py runs it on.

The rule per (frame f, node m): camera-space point = node @ view[:3, :3] + view[3, :3]; (row, col) = (fy y / z + cy,
fx x / z + cx); both truncated toward zero; row >= H -> H - 1 and col >= W -> W - 1, after that anything < 0 -> 0; the label is
map[row, col], 0 for a camera without a map.  The median is the LOWER one over the frames: np.sort(...)[(F - 1) // 2]."""
import math

import numpy as np


class Camera:
    """What node_semantic_labels reads of a camera.  ``world_view_transform`` is a numpy (4, 4) here (row-vector convention:
    the translation in the last ROW); the test hands torch tensors over."""

    def __init__(self, view, H, W, fx, fy, semantic_seg=None, K=None):
        self.world_view_transform = np.asarray(view, dtype=np.float32)
        self.image_height, self.image_width = int(H), int(W)
        # the field of view that gives back these focal lengths: fx = W / (2 tan(FoVx / 2))
        self.FoVx, self.FoVy = 2.0 * math.atan(W / (2.0 * fx)), 2.0 * math.atan(H / (2.0 * fy))
        self.semantic_seg = semantic_seg
        self.K = K


def intrinsics(cam):
    """fx, fy, cx, cy as project_nodes_to_2d_elements forms them, in float64."""
    H, W = cam.image_height, cam.image_width
    fy, fx = H / (2 * math.tan(cam.FoVy * 0.5)), W / (2 * math.tan(cam.FoVx * 0.5))
    if cam.K is not None:
        return fx, fy, float(cam.K[0][2]), float(cam.K[1][2])
    return fx, fy, W / 2, H / 2


def project(cam, nodes, dtype):
    """(M, 2) (row, col) of ``nodes`` (M, 3) in ``dtype`` arithmetic, one rounding per operation in the kernel's order."""
    t = np.dtype(dtype).type
    V = np.asarray(cam.world_view_transform).astype(dtype)
    p = np.asarray(nodes).astype(dtype)
    fx, fy, cx, cy = (t(v) for v in intrinsics(cam))
    cam_space = [p[:, 0] * V[0, k] + p[:, 1] * V[1, k] + p[:, 2] * V[2, k] + V[3, k] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        row = fy * cam_space[1] / cam_space[2] + cy
        col = fx * cam_space[0] / cam_space[2] + cx
    return np.stack([row, col], axis=-1)


def pixels(cam, proj):
    """Truncate toward zero, then the clamps in the stated order.  Returns ``(rows, cols, hits)``: ``hits`` counts how often
    each of the three clamps acted (row >= H, col >= W, < 0)."""
    H, W = cam.image_height, cam.image_width
    pos = np.trunc(proj).astype(np.int64)
    hit_h, hit_w = pos[:, 0] >= H, pos[:, 1] >= W
    pos[hit_h, 0] = H - 1
    pos[hit_w, 1] = W - 1
    neg = pos < 0
    pos[neg] = 0
    return pos[:, 0], pos[:, 1], np.array([hit_h.sum(), hit_w.sum(), neg.sum()])


def labels_and_median(d_nodes, cameras, dtype=np.float64):
    """``(labels (F, M) float32, median (M,) int32, hits (3,))`` of d_nodes (F, M, 3) with the projection in ``dtype``."""
    F, M = d_nodes.shape[:2]
    labels = np.zeros((F, M), dtype=np.float32)
    hits = np.zeros(3, dtype=np.int64)
    for f, cam in enumerate(cameras):
        if cam.semantic_seg is None:
            continue
        rows, cols, h = pixels(cam, project(cam, d_nodes[f], dtype))
        hits += h
        labels[f] = np.asarray(cam.semantic_seg)[rows, cols].astype(np.float32)
    return labels, np.sort(labels, axis=0)[(F - 1) // 2].astype(np.int32), hits


def distance_to_integer(d_nodes, cameras):
    """The smallest distance of any (f, m) projection coordinate, in float64, to an integer — over ALL pairs, cameras without a
    map included."""
    worst = np.inf
    for f, cam in enumerate(cameras):
        p = project(cam, d_nodes[f], np.float64)
        worst = min(worst, float(np.abs(p - np.round(p)).min()))
    return worst


# ---- scenes: every projection lies on a quarter-pixel lattice, a quarter or more from any integer -------------------------
# the 24 proper rotations that map the axes onto each other would do; these six (with a reflection or not — the kernel takes
# any matrix) exercise every entry of the 3 x 3 block
_ROTATIONS = (((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1), (1, 0, 0)), ((0, 0, 1), (1, 0, 0), (0, 1, 0)),
              ((-1, 0, 0), (0, 0, 1), (0, 1, 0)), ((0, -1, 0), (1, 0, 0), (0, 0, 1)), ((0, 0, -1), (0, 1, 0), (1, 0, 0)))
_SHAPES = ((7, 5, 4.0, 8.0), (40, 64, 32.0, 16.0), (33, 17, 16.0, 16.0), (12, 20, 8.0, 4.0))  # H, W, fx, fy (powers of two)
_DEPTHS = np.array([1.0, 1.25, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0])


def scene(F, M, seed, null_every=0, null_keep=0):
    """``(d_nodes (F, M, 3) float32, cameras)``.  Camera f has one of four image shapes (7 x 5 and 40 x 64 among them), a signed
    axis permutation as rotation and a translation on a grid of 1 / 8; every third camera carries ``K`` with a principal point
    off the centre.  Node (f, m) is placed in camera f's space at depth z in [1, 4] (multiples of 1 / 4) and at
    x = z (2 i + 1) / (4 fx), y = z (2 j + 1) / (4 fy), so that fx x / z and fy y / z are odd multiples of 1 / 4 — exactly, in
    float32 too: every factor is a small dyadic number — and the principal points are multiples of 1 / 2 or of 1 / 8 off them:
    no projection comes nearer than 1 / 8 to an integer.  i and j range so that rows run from about -H / 2 to 3 H / 2 (and
    columns likewise): all three clamps act.  Maps hold labels in [-9, -1], one small label on half of the pixels, and labels in
    [2^19, 2^20].
    Cameras without a map: ``null_every`` = k > 0 removes the map of every camera whose index is not a multiple of k when
    ``null_keep`` is 0 (a majority for k >= 3), or of every camera whose index IS a multiple of k otherwise (a minority)."""
    rng = np.random.default_rng(seed)
    cameras, frames = [], []
    for f in range(F):
        H, W, fx, fy = _SHAPES[(f + seed) % len(_SHAPES)]
        R = np.array(_ROTATIONS[(f + 2 * seed) % len(_ROTATIONS)], dtype=np.float64)  # p_cam = p_world @ R + T
        T = rng.integers(-16, 17, 3) / 8.0
        view = np.zeros((4, 4))
        view[:3, :3], view[3, :3], view[3, 3] = R, T, 1.0
        K = None
        if f % 3 == 1:
            K = np.array([[fx, 0.0, W / 2 + 1.125], [0.0, fy, H / 2 - 0.625], [0.0, 0.0, 1.0]])
        seg, u = rng.integers(2 ** 19, 2 ** 20 + 1, (H, W)).astype(np.int32), rng.random((H, W))
        seg[u < 0.5] = rng.integers(1, 6)  # (half of the map one small label, so that medians are not all distinct)
        seg[u > 0.8] = rng.integers(-9, 0, int((u > 0.8).sum()))
        seg[0, 0], seg[H - 1, W - 1] = 2 ** 20, -9  # (the corners, where the clamps send many nodes)
        if null_every and ((f % null_every != 0) if not null_keep else (f % null_every == 0)):
            seg = None
        cameras.append(Camera(view, H, W, fx, fy, seg, K))
        z = rng.choice(_DEPTHS, M)
        i = rng.integers(-3 * W, 3 * W, M)  # fx x / z = (2 i + 1) / 4 in [-3 W / 2, 3 W / 2): columns from about -W to 2 W
        j = rng.integers(-3 * H, 3 * H, M)  # rows from about -H to 2 H
        p_cam = np.stack([z * (2 * i + 1) / (4 * fx), z * (2 * j + 1) / (4 * fy), z], axis=-1)
        frames.append((p_cam - T) @ R.T)  # (R is orthogonal with entries 0, +-1: exact)
    d_nodes = np.stack(frames)
    assert np.array_equal(d_nodes.astype(np.float32).astype(np.float64), d_nodes)  # the nodes are float32 numbers
    return d_nodes.astype(np.float32), cameras
