"""The evaluation report's definitions in plain torch ops (on the CPU in the tests): PSNR, L1, ``piq.ssim`` and ``pytorch_msssim.ms_ssim`` as
``riggs_amd.metrics`` documents them, restated from the two packages' published algorithms (neither package is a dependency).
``dtype=torch.float64`` is the reference the HIP kernels are compared with; ``dtype=torch.float32`` is the same sequence of ops
as the packages issue them, and its distance from the float64 form is what the float32 evaluation of the cancelling
``E[x^2] - mu^2`` costs (the yardstick of the GPU test's tolerance)."""
import numpy as np
import torch
import torch.nn.functional as F

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=torch.float64):
    """``exp(-(k - 5)^2 / (2 1.5^2))`` normalised to sum 1 in float64, then rounded to ``dtype``."""
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(k * k) / (2 * 1.5 * 1.5))
    return (g / g.sum()).to(dtype)


def pool_factor(H, W):
    """piq's ``max(1, round(min(H, W) / 256))`` — Python's round: half to even."""
    return max(1, round(min(H, W) / 256))


def pool(x, k, pad_h=0, pad_w=0):
    """Mean pool of (B, C, h, w), kernel = stride = k, ``pad`` zeros in front that count in the divisor; windows the image does
    not fill are dropped."""
    x = F.pad(x, (pad_w, 0, pad_h, 0))
    B, C, h, w = x.shape
    oh, ow = h // k, w // k
    v = x[:, :, :oh * k, :ow * k].reshape(B, C, oh, k, ow, k)
    acc = torch.zeros(B, C, oh, ow, dtype=x.dtype, device=x.device)
    for di in range(k):
        for dj in range(k):
            acc = acc + v[:, :, :, di, :, dj]
    return acc / (k * k)


def _filter(x, win):
    """The valid separable filter, per channel: along the rows' direction (W) first, then along H."""
    C = x.shape[1]
    x = F.conv2d(x, win.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(x, win.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)


def level(x, y, dtype=torch.float64):
    """``(ssim_c, cs_c)`` of one level, each (B, C): the means of ssim_map and cs_map over the valid outputs."""
    win = window(dtype).to(x.device)
    mu1, mu2 = _filter(x, win), _filter(y, win)
    s1 = _filter(x * x, win) - mu1 * mu1
    s2 = _filter(y * y, win) - mu2 * mu2
    s12 = _filter(x * y, win) - mu1 * mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def metrics_torch(x, y, clamp=True, ms_ssim=True, dtype=torch.float64):
    """The report of (B, C, H, W) tensors in plain torch ops on their device: ``(out (B, 4), levels (B, 6, C, 2), mse (B,),
    relu_inputs (B, C, 5))`` in ``dtype``."""
    x, y = x.to(dtype), y.to(dtype)
    if clamp:
        x, y = x.clamp(0.0, 1.0), y.clamp(0.0, 1.0)
    B, C, H, W = x.shape
    new = dict(dtype=dtype, device=x.device)
    levels = torch.full((B, 6, C, 2), float("nan"), **new)
    d = x - y
    l1 = d.abs().flatten(1).mean(1)
    mse = (d * d).flatten(1).mean(1)
    psnr = 20 * torch.log10(1.0 / torch.sqrt(mse))
    f = pool_factor(H, W)
    lx, ly = x, y
    n_ms = 5 if ms_ssim else 1
    if ms_ssim and min(H, W) <= 160:
        raise ValueError("MS-SSIM needs min(H, W) > 160")
    for l in range(n_ms):
        s, c = level(lx, ly, dtype)
        levels[:, l, :, 0], levels[:, l, :, 1] = s, c
        if l < n_ms - 1:
            ph, pw = lx.shape[2] % 2, lx.shape[3] % 2
            lx, ly = pool(lx, 2, ph, pw), pool(ly, 2, ph, pw)
    if f > 1:
        s, c = level(pool(x, f), pool(y, f), dtype)
        levels[:, 5, :, 0], levels[:, 5, :, 1] = s, c
    else:
        levels[:, 5] = levels[:, 0]
    ssim = levels[:, 5, :, 0].mean(1)
    if ms_ssim:
        v = torch.cat([levels[:, :4, :, 1], levels[:, 4:5, :, 0]], 1)           # (B, 5, C)
        wt = torch.tensor(MS_WEIGHTS, **new).view(1, 5, 1)
        ms = torch.prod(torch.relu(v) ** wt, dim=1).mean(1)
        relu_inputs = v.permute(0, 2, 1)
    else:
        ms = torch.full((B,), float("nan"), **new)
        relu_inputs = torch.full((B, C, 5), float("nan"), **new)
    return torch.stack([l1, psnr, ssim, ms], 1), levels, mse, relu_inputs


def image_metrics(x, y, clamp=True, ms_ssim=True, dtype=torch.float64):
    """``x``, ``y``: (B, C, H, W) arrays.  Returns a dict of float64 NumPy arrays: ``out`` (B, 4) = [l1, psnr, ssim, ms_ssim],
    ``levels`` (B, 6, C, 2) = [ssim mean, cs mean] of the five MS-SSIM levels and the piq level (NaN where not computed),
    ``mse`` (B,) and ``relu_inputs`` (B, C, 5): what MS-SSIM passes through relu."""
    r = metrics_torch(torch.as_tensor(np.asarray(x)), torch.as_tensor(np.asarray(y)), clamp, ms_ssim, dtype)
    return {k: t.to(torch.float64).numpy() for k, t in zip(("out", "levels", "mse", "relu_inputs"), r)}


# ---- the seeded cases of tests/test_metrics_cpu.py, tests/test_gpu_metrics.py and tests/golden/metrics_expected.json ----------
MS_SHAPES = ((3, 161, 161), (3, 176, 163), (1, 200, 333), (3, 385, 390), (1, 640, 641), (1, 700, 650))
TILE_H, TILE_W = 64, 32  # the level kernel's output tile (csrc/metrics.hip: MT_TH x MT_T)
PLAIN_SHAPES = ((3, 11, 11), (1, 11, 75), (2, 43, 12)) + tuple((1, TILE_H + d, TILE_W + d) for d in (0, 1, 10, 11))
PAIRS = ("noisy", "uniform", "negative")
SEED = 20240


def _bilinear(grid, H, W):
    """(C, gh, gw) -> (C, H, W), corners aligned."""
    C, gh, gw = grid.shape
    ys, xs = np.linspace(0, gh - 1, H), np.linspace(0, gw - 1, W)
    y0, x0 = np.minimum(ys.astype(int), gh - 2), np.minimum(xs.astype(int), gw - 2)
    fy, fx = (ys - y0)[None, :, None], (xs - x0)[None, None, :]
    g = lambda a, b: grid[:, a][:, :, b]  # noqa: E731
    return (g(y0, x0) * (1 - fy) * (1 - fx) + g(y0, x0 + 1) * (1 - fy) * fx
            + g(y0 + 1, x0) * fy * (1 - fx) + g(y0 + 1, x0 + 1) * fy * fx)


def make_pair(shape, pair, seed=SEED):
    """One seeded float32 (1, C, H, W) pair: ``noisy`` = a smooth image (bilinear upsampling of an (H/8+2, W/8+2) random
    grid) against itself plus 0.08 Gaussian noise, clamped; ``uniform`` = two independent uniform images; ``negative`` = the
    smooth image against 1 - itself."""
    C, H, W = shape
    rng = np.random.default_rng([seed, C, H, W])
    smooth = _bilinear(rng.random((C, H // 8 + 2, W // 8 + 2)), H, W)
    noise = rng.normal(0.0, 0.08, (C, H, W))
    u1, u2 = rng.random((C, H, W)), rng.random((C, H, W))
    smooth = np.float32(smooth)
    if pair == "noisy":
        x, y = smooth, np.float32(np.clip(smooth + noise, 0.0, 1.0))
    elif pair == "uniform":
        x, y = np.float32(u1), np.float32(u2)
    elif pair == "negative":
        x, y = smooth, np.float32(1.0) - smooth
    else:
        raise KeyError(pair)
    return np.ascontiguousarray(x[None]), np.ascontiguousarray(y[None])


def cases():
    """(name, shape, pair, ms_ssim) of every seeded case."""
    out = []
    for shapes, ms in ((MS_SHAPES, True), (PLAIN_SHAPES, False)):
        for shape in shapes:
            for pair in PAIRS:
                out.append(("%dx%dx%d_%s" % (shape + (pair,)), shape, pair, ms))
    return out


def tolerance(dev32):
    """What the HIP result may deviate from the float64 form, given the float32 form's deviation: 4x (another summation order and
    contraction in an equally precise evaluation), at least 1e-6."""
    return max(4.0 * float(dev32), 1e-6)

