"""2-D skeleton thinning of silhouette masks on csrc/thin.hip: what the reference makes offline with
``skimage.morphology.thin`` (process_data/cal_2d_skeleton.py -> ``train_thinned/*.png``), reads back with ``np.where``
(scene/dataset_readers.py) and divides by ``args.resolution`` (utils/camera_utils.py:60) to get ``viewpoint_cam.thinned`` — the
pixel set ``riggs_amd.loss.cal_skeleton_loss`` and ``node_projection_loss`` compare the projected skeleton with.

The algorithm is Guo and Hall's two-subiteration parallel thinning, restated from its published definition (the conditions are
written out in csrc/thin.hip and tests/thin_ref.py).  It reproduces the published 7 x 7 example of ``thin``'s documentation;
scikit-image was not available where this was written, so agreement with an installed skimage beyond that example is NOT verified.

Everything runs on the device; CPU tensors are refused, there is no CPU path."""
from __future__ import annotations

import torch

from . import _lib as L

PATH_AUTO, PATH_LDS, PATH_GLOBAL = (L.CONSTANTS["RIGGS_THIN_PATH_" + k] for k in ("AUTO", "LDS", "GLOBAL"))


def _masks(name, image):
    """``image`` (H, W) or (B, H, W), on the device, real or bool -> contiguous uint8 (B, H, W) of ``image > 0``."""
    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise L.RiggsHipError("%s: the image must be a CUDA(HIP) tensor — there is no CPU path" % name)
    if image.dim() not in (2, 3) or image.numel() == 0 or image.is_complex():
        raise L.RiggsHipError("%s takes a non-empty real (H, W) or (B, H, W) image, got %s %s" % (name, tuple(image.shape), image.dtype))
    x = image.detach()
    x = x if x.dtype is torch.bool else x > 0
    return x.reshape((-1,) + tuple(x.shape[-2:])).contiguous().view(torch.uint8)


def thin(image, max_num_iter=None, *, _path=None, _check_every=8, _first_subiter=0, _max_subiters=None):
    """``skimage.morphology.thin(image > 0, max_num_iter)`` of one (H, W) image or of each image of a (B, H, W) batch: a bool
    tensor of the same shape holding the one-pixel-wide skeleton.  ``max_num_iter``: the number of iterations (of two
    sub-iterations each) at most; ``None`` (or 0, as in skimage) runs until nothing changes.

    Images whose bit plane fits one workgroup's LDS (``riggs_thin_path``: 800 x 800 does, about 995 x 1280 is the limit) take
    one launch for the whole batch and never synchronise; larger ones run one launch per sub-iteration and read a device
    counter back every ``_check_every`` iterations.  The underscored keywords are for the tests: ``_path`` forces a path,
    ``_first_subiter`` starts with the second table, ``_max_subiters`` bounds single sub-iterations."""
    x = _masks("thin", image)
    B, H, W = x.shape
    if _max_subiters is None:
        if max_num_iter is not None and max_num_iter < 0:
            raise L.RiggsHipError("thin: max_num_iter must be positive (or None)")
        unbounded = not max_num_iter or max_num_iter == float("inf") or max_num_iter >= 2 ** 30
        _max_subiters = -1 if unbounded else 2 * int(max_num_iter)
    lib = L.lib()
    path = PATH_AUTO if _path is None else int(_path)
    out = torch.empty_like(x)
    nbytes = int(lib.riggs_thin_workspace_bytes(B, H, W, path))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    with torch.cuda.device(x.device):
        L.check(lib.riggs_thin(B, H, W, x.data_ptr(), out.data_ptr(), int(_first_subiter), int(_max_subiters), path,
                               int(_check_every), L.ptr(ws), L.stream_ptr()), "riggs_thin")
    return out.view(torch.bool).reshape(image.shape)


def thinned_elements(masks, resolution=1, capacity=None):
    """The set (``> 0``) pixels of one (H, W) image or of each of (B, H, W) — usually ``thin(...)``'s output — as
    ``(points (B, capacity, 2) float32, counts (B,) int32)``: ``points[b, :counts[b]]`` are the (row, col) coordinates divided
    by ``resolution`` (in float64, then rounded to float32, as the reference does), in ``np.where``'s row-major order; rows at and
    beyond ``counts[b]`` are left as allocated (zero).  ``points[b]`` with ``pixel_count=counts[b]`` is the ``thinned`` /
    ``pixel_count`` pair ``cal_skeleton_loss``, ``node_projection_loss`` and ``GraphedTrainStep`` take.

    ``capacity`` defaults to the largest count (at least 1), which costs one host read; passing it avoids the read — counts are
    then capped at it."""
    x = _masks("thinned_elements", masks)
    B, H, W = x.shape
    if not float(resolution) > 0:
        raise L.RiggsHipError("thinned_elements: resolution must be positive")
    if capacity is None:
        capacity = max(int(x.sum(dim=(1, 2), dtype=torch.int64).max().item()), 1)
    capacity = int(capacity)
    if capacity < 0 or capacity >= 2 ** 31:
        raise L.RiggsHipError("thinned_elements: capacity must be in [0, 2^31)")
    points = torch.zeros(B, capacity, 2, dtype=torch.float32, device=x.device)
    counts = torch.empty(B, dtype=torch.int32, device=x.device)
    elements_into(x, resolution, points, counts)
    return points, counts


def elements_into(masks, resolution, points, counts):
    """``thinned_elements`` into caller-owned buffers: ``points`` (B, capacity, 2) float32 and ``counts`` (B,) int32, both
    contiguous on the masks' device.  Only ``points[b, :counts[b]]`` and ``counts`` are written."""
    x = _masks("elements_into", masks)
    B, H, W = x.shape
    L.require_cuda_f32("points", points, (B, None, 2))
    if not (points.is_contiguous() and counts.is_cuda and counts.dtype is torch.int32 and counts.is_contiguous() and counts.numel() == B):
        raise L.RiggsHipError("elements_into: points must be contiguous (B, capacity, 2) float32 and counts contiguous (B,) int32 on the device")
    with torch.cuda.device(x.device):
        L.check(L.lib().riggs_thin_elements(B, H, W, x.data_ptr(), float(resolution), int(points.shape[1]), points.data_ptr(),
                                            counts.data_ptr(), L.stream_ptr()), "riggs_thin_elements")


def get_2d_skeleton(mask):
    """process_data/cal_2d_skeleton.py::get_2d_skeleton: the skeleton of ``mask > 0`` as an int32 image of 0 / 255 (on the
    device; the reference returns a NumPy array)."""
    return thin(mask).to(torch.int32) * 255


def extract_skeleton(masks):
    """process_data/cal_2d_skeleton.py::extract_skeleton: ``masks`` (B, 1, H, W) -> the list of the B images
    ``get_2d_skeleton(masks[b, 0])``, thinned in one batch."""
    if not isinstance(masks, torch.Tensor) or masks.dim() != 4:
        raise L.RiggsHipError("extract_skeleton takes (B, 1, H, W) masks")
    return list(get_2d_skeleton(masks[:, 0]).unbind(0))


def camera_thinned(gt_alpha_mask, resolution=1):
    """The (M, 2) float32 tensor ``Camera.thinned`` holds, from the camera's alpha mask (H, W) or (1, H, W): the (row, col) pixels
    of its skeleton divided by ``resolution``.  One host read (M)."""
    if isinstance(gt_alpha_mask, torch.Tensor) and gt_alpha_mask.dim() == 3 and gt_alpha_mask.shape[0] == 1:
        gt_alpha_mask = gt_alpha_mask[0]
    if not isinstance(gt_alpha_mask, torch.Tensor) or gt_alpha_mask.dim() != 2:
        raise L.RiggsHipError("camera_thinned takes one (H, W) or (1, H, W) mask")
    points, counts = thinned_elements(thin(gt_alpha_mask), resolution)
    return points[0, :int(counts.item())]
