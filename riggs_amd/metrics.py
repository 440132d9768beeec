"""The evaluation report: PSNR, L1, SSIM and MS-SSIM of rendered frames against their ground truth, as
``skeleton_training_report`` (train_utils.py:56-243) and ``render_set`` (render_rig.py:111-218) compute them, on HIP kernels
(csrc/metrics.hip).  Inference only: everything runs under ``torch.no_grad``.

Neither of the two packages the reference takes its SSIMs from is a dependency of this library.  Both definitions are
RESTATED here from the packages' published algorithms, and the numbers are pinned to this restatement (tests/metrics_ref.py is
its float64 form), not to an import.

Per level and channel, with ``G*`` the valid (no padding) separable 11-tap Gaussian filter of sigma 1.5, ``C1 = 0.01^2``,
``C2 = 0.03^2``::

    mu1 = G*x, mu2 = G*y, s1 = G*(x x) - mu1^2, s2 = G*(y y) - mu2^2, s12 = G*(x y) - mu1 mu2
    cs_map   = (2 s12 + C2) / (s1 + s2 + C2)
    ssim_map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs_map
    ssim_c, cs_c = their means over the (h - 10) x (w - 10) valid outputs

``piq.ssim(x, y, data_range=1.)`` (utils/image_utils.py:35): mean-pool both images by ``f = max(1, round(min(H, W) / 256))``
(Python's round: half to even), one level, the mean of ``ssim_c`` over the channels.

``pytorch_msssim.ms_ssim(X, Y, data_range=1.)``: needs ``min(H, W) > 160``; levels 0..4 with a 2 x 2 mean pool between them
(``(h % 2, w % 2)`` zeros in front, counted in the divisor); ``v_l = relu(cs_c)`` for l = 0..3 and ``v_4 = relu(ssim_c)`` of
level 4; per channel ``prod_l v_l ^ wt_l`` with ``wt = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]``; the mean over the channels.

``psnr`` (utils/image_utils.py:30-32): ``20 log10(1 / sqrt(mean (x - y)^2))`` per frame (``inf`` for identical images);
``l1``: ``mean |x - y|``.

This is NOT the training loss's SSIM (``riggs_amd.loss.ssim`` = utils/loss_utils.ssim: a zero-padded window, no pooling).
LPIPS needs network weights that are not part of this library: ``evaluate`` takes optional callables for it."""
from __future__ import annotations

import torch

from . import _lib as L

COLUMNS = ("l1", "psnr", "ssim", "lpips", "ms_ssim", "alex_lpips")  # the per-frame table of ``evaluate``


def _bchw(t, name):
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise L.RiggsHipError("%s must be (B, C, H, W) or (C, H, W), got %s" % (name, tuple(t.shape)))
    return L.require_cuda_f32(name, t.detach())


@torch.no_grad()
def image_metrics(images, gts, clamp=True, ms_ssim=True, return_levels=False):
    """``(B, 4)`` = ``[l1, psnr, ssim, ms_ssim]`` per frame of ``images`` against ``gts`` (both (B, C, H, W) or (C, H, W),
    float32 on the device), everything from ONE C call: level 0 is shared between PSNR, L1, MS-SSIM and — when the pooling
    factor is 1 — SSIM.  ``clamp=True`` clamps both to [0, 1] first, as the reference does before its metrics.  With
    ``ms_ssim=False`` that column is NaN and no size limit applies; with ``ms_ssim=True`` and ``min(H, W) <= 160`` it raises
    ``ValueError``.  ``return_levels=True`` also returns ``(B, 6, C, 2)``: ``[ssim mean, cs mean]`` per channel of the five
    MS-SSIM levels and of the piq level (NaN for a level that was not computed).  A frame's row does not depend on the batch
    it is scored in.  No host synchronisation."""
    x, y = _bchw(images, "images"), _bchw(gts, "gts")
    if x.shape != y.shape:
        raise L.RiggsHipError("images %s and gts %s differ in shape" % (tuple(x.shape), tuple(y.shape)))
    B, C, H, W = x.shape
    if ms_ssim and min(H, W) <= 160:
        raise ValueError("MS-SSIM needs min(H, W) > 160 (five levels of an 11-tap window), got %d x %d" % (H, W))
    lib = L.lib()
    n_ws = int(lib.riggs_image_metrics_workspace_floats(B, C, H, W))
    ws = torch.empty(max(n_ws, 2), dtype=torch.float32, device=x.device)
    out = torch.empty(B, 4, dtype=torch.float32, device=x.device)
    levels = torch.empty(B, 6, C, 2, dtype=torch.float32, device=x.device) if return_levels else None
    L.check(lib.riggs_image_metrics(B, C, H, W, x.data_ptr(), y.data_ptr(), int(bool(clamp)), int(bool(ms_ssim)), out.data_ptr(),
                                    L.ptr(levels), ws.data_ptr(), ws.numel(), L.stream_ptr()), "riggs_image_metrics")
    return (out, levels) if return_levels else out


def psnr(img1, img2):
    """``utils.image_utils.psnr``: (B, 1), no clamping."""
    return image_metrics(img1, img2, clamp=False, ms_ssim=False)[:, 1:2]


def ssim(x, y, kernel_size=11, kernel_sigma=1.5, data_range=1.0, reduction="mean", full=False, downsample=True, k1=0.01,
         k2=0.03):
    """``utils.image_utils.ssim`` (= ``piq.ssim``) with the reference's call: ``reduction`` "mean" (a scalar) or "none" ((B,));
    a ``data_range`` other than 1 divides the inputs first; any other option of the package raises ``NotImplementedError``."""
    if (kernel_size, kernel_sigma, full, downsample, k1, k2) != (11, 1.5, False, True, 0.01, 0.03):
        raise NotImplementedError("the HIP kernels implement piq.ssim's defaults: kernel_size=11, kernel_sigma=1.5, full=False, "
                                  "downsample=True, k1=0.01, k2=0.03")
    if reduction not in ("mean", "none"):
        raise NotImplementedError("reduction must be 'mean' or 'none'")
    if float(data_range) != 1.0:
        x, y = x / float(data_range), y / float(data_range)
    col = image_metrics(x, y, clamp=False, ms_ssim=False)[:, 2]
    return col.mean(dim=0) if reduction == "mean" else col


def ms_ssim(X, Y, data_range=1.0, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """``pytorch_msssim.ms_ssim`` with the reference's call; ``size_average=False`` gives (B,)."""
    if (win_size, win_sigma, win, weights, tuple(K)) != (11, 1.5, None, None, (0.01, 0.03)):
        raise NotImplementedError("the HIP kernels implement pytorch_msssim.ms_ssim's defaults: win_size=11, win_sigma=1.5, "
                                  "the five default weights, K=(0.01, 0.03)")
    if float(data_range) != 1.0:
        X, Y = X / float(data_range), Y / float(data_range)
    col = image_metrics(X, Y, clamp=False, ms_ssim=True)[:, 3]
    return col.mean() if size_average else col


@torch.no_grad()
def evaluate(cameras, gaussians, skeleton, pipe, background, lpips_fn=None, alex_lpips_fn=None, chunk=8, d_rot_as_res=True):
    """The loop of ``skeleton_training_report`` / ``render_set`` over ``cameras``: per camera the skeleton's deformation at
    ``cam.fid`` (``d_scaling`` zeroed, ``d_rotation`` too for isotropic Gaussians), ``render(...)["render"]``; the frames are
    collected ``chunk`` at a time (cameras of differing sizes go into separate chunks) and scored by one ``image_metrics`` call
    with ``clamp=True`` against the cameras' ``original_image``.  ``lpips_fn`` / ``alex_lpips_fn``: optional callables given
    the clamped ``(1, 3, H, W)`` pair; their columns are NaN when absent.  One device-to-host copy, at the end.

    Returns ``(table, means)``: ``table`` a float64 (n, 6) CPU tensor with the columns ``COLUMNS`` and ``means`` a dict of
    their means (the reference's ``torch.stack(list).mean()``)."""
    from .render import render
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    rows, extra = [], []
    frames, gts = [], []

    def flush():
        if frames:
            rows.append(image_metrics(torch.stack(frames), torch.stack(gts), clamp=True, ms_ssim=True))
            frames.clear()
            gts.clear()

    for cam in cameras:
        xyz = gaussians.get_xyz
        time_input = skeleton.deform.expand_time(cam.fid)
        d = skeleton.step(xyz.detach(), time_input, motion_mask=gaussians.motion_mask)
        d_rotation, d_scaling = d["d_rotation"], d["d_scaling"]
        d_scaling = torch.zeros_like(d_scaling) if isinstance(d_scaling, torch.Tensor) else 0.0
        if gaussians.use_isotropic_gs:
            d_rotation = torch.zeros_like(d_rotation) if isinstance(d_rotation, torch.Tensor) else 0.0
        image = render(cam, gaussians, pipe, background, d["d_xyz"], d_rotation, d_scaling, d_opacity=d.get("d_opacity"),
                       d_color=d.get("d_color"), d_rot_as_res=d_rot_as_res)["render"]
        gt = cam.original_image.to(image.device, torch.float32)
        if frames and frames[0].shape != image.shape:
            flush()
        frames.append(image)
        gts.append(gt)
        if lpips_fn is not None or alex_lpips_fn is not None:
            a, b = image.clamp(0.0, 1.0)[None], gt.clamp(0.0, 1.0)[None]
            nan = torch.full((), float("nan"), device=image.device)
            f = lambda fn: nan if fn is None else torch.as_tensor(fn(a, b), device=image.device).float().mean()  # noqa: E731
            extra.append(torch.stack([f(lpips_fn), f(alex_lpips_fn)]))
        if len(frames) == chunk:
            flush()
    flush()
    if not rows:
        raise ValueError("evaluate: no cameras")
    dev = torch.cat(rows)                                           # (n, 4): l1, psnr, ssim, ms_ssim
    lp = torch.stack(extra) if extra else torch.full((dev.shape[0], 2), float("nan"), device=dev.device)
    table = torch.stack([dev[:, 0], dev[:, 1], dev[:, 2], lp[:, 0], dev[:, 3], lp[:, 1]], 1).double().cpu()
    means = {name: float(table[:, i].mean()) for i, name in enumerate(COLUMNS)}
    return table, means


def write_numerical_res(path, table, means):
    """The file of render_rig.py:211-217: the same header line, format strings and ``mean`` row.  ``table``: (n, 6) with the
    columns ``COLUMNS`` (what ``evaluate`` returns); ``means``: its dict."""
    rows = [[float(v) for v in r] for r in (table.tolist() if hasattr(table, "tolist") else table)]
    i = {name: k for k, name in enumerate(COLUMNS)}
    order = ("psnr", "ssim", "lpips", "ms_ssim", "alex_lpips")
    with open(path, "w") as fid:
        print('ID\tpsnr\tssim\tlpips\tms_ssim\talex_lpips', file=fid)
        for n, r in enumerate(rows):
            print('%d\t%.2f\t%.4f\t%.4f\t%.4f\t%.4f' % ((n,) + tuple(r[i[k]] for k in order)), file=fid)
        print('mean\t%.2f\t%.4f\t%.4f\t%.4f\t%.4f' % tuple(float(means[k]) for k in order), file=fid)

