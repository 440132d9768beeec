"""CPU: the evaluation report's definitions (tests/metrics_ref.py, the float64 restatement riggs_amd.metrics is pinned to) against
independent forms and its recorded values; the C entry's argument validation; the report file.  No GPU."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as MR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_expected.json")


def _piq_level_numpy(x, y):
    """One level the way piq writes it, in NumPy/SciPy float64: the 2-D window is the outer product of the normalised 1-D one
    (piq's ``gaussian_filter``: ``g = exp(-(coords^2) / (2 sigma^2)); g /= g.sum(); (g[None] * g[:, None])``), correlated with
    no padding."""
    from scipy.signal import correlate2d
    k = np.arange(11, dtype=np.float64) - 5
    g = np.exp(-(k ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    win = g[None, :] * g[:, None]
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    out = []
    for cx, cy in zip(x, y):
        f = lambda a: correlate2d(a, win, "valid")  # noqa: E731
        mu_x, mu_y = f(cx), f(cy)
        mu_xx, mu_yy, mu_xy = mu_x ** 2, mu_y ** 2, mu_x * mu_y
        s_xx, s_yy, s_xy = f(cx ** 2) - mu_xx, f(cy ** 2) - mu_yy, f(cx * cy) - mu_xy
        cs = (2 * s_xy + c2) / (s_xx + s_yy + c2)
        ss = (2 * mu_xy + c1) / (mu_xx + mu_yy + c1) * cs
        out.append((ss.mean(), cs.mean()))
    return np.array(out)


@pytest.mark.parametrize("shape,pair", [((3, 43, 57), "noisy"), ((1, 11, 11), "uniform"), ((2, 64, 31), "negative")])
def test_level_equals_the_scipy_form(shape, pair):
    x, y = MR.make_pair(shape, pair)
    s, c = MR.level(torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64))
    want = _piq_level_numpy(np.float64(x[0]), np.float64(y[0]))
    assert np.abs(s[0].numpy() - want[:, 0]).max() <= 1e-12
    assert np.abs(c[0].numpy() - want[:, 1]).max() <= 1e-12


@pytest.mark.parametrize("h,w", [(20, 20), (21, 20), (20, 23), (161, 163), (11, 12)])
def test_pool_matches_avg_pool2d(h, w):
    x = torch.rand(2, 3, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(h * 1000 + w))
    ph, pw = h % 2, w % 2
    want = torch.nn.functional.avg_pool2d(x, kernel_size=2, padding=(ph, pw), count_include_pad=True)
    got = MR.pool(x, 2, ph, pw)
    assert got.shape == want.shape == (2, 3, (h + 1) // 2, (w + 1) // 2)
    assert float((got - want).abs().max()) <= 1e-15
    if ph and not pw:  # the first output row is (0 + x[0]) / 2 and the pairs are (x[2i-1], x[2i])
        assert float((got[:, :, 0] - (x[:, :, 0, 0::2] + x[:, :, 0, 1::2]) / 4).abs().max()) <= 1e-15
        pairs = (x[:, :, 1::2] + x[:, :, 2::2]) / 2
        assert float((got[:, :, 1:] - (pairs[..., 0::2] + pairs[..., 1::2]) / 2).abs().max()) <= 1e-15
    for f in (2, 3):
        want = torch.nn.functional.avg_pool2d(x, kernel_size=f)
        got = MR.pool(x, f)
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-15


def test_pool_factor_rounds_half_to_even():
    assert [MR.pool_factor(m, m + 7) for m in (383, 384, 640, 641, 896)] == [1, 2, 2, 3, 4]
    assert MR.pool_factor(900, 100) == 1


def test_identical_images():
    x, _ = MR.make_pair((3, 176, 163), "uniform")
    r = MR.image_metrics(x, x)
    assert r["out"][0, 0] == 0.0 and r["out"][0, 1] == math.inf
    assert abs(r["out"][0, 2] - 1.0) <= 1e-12 and abs(r["out"][0, 3] - 1.0) <= 1e-12


def test_negative_image_has_zero_ms_ssim():
    x, y = MR.make_pair((3, 176, 163), "negative")
    r = MR.image_metrics(x, y)
    assert r["out"][0, 3] == 0.0 and r["out"][0, 2] < 0
    assert MR.image_metrics(x, y, dtype=torch.float32)["out"][0, 3] == 0.0


def test_ms_ssim_needs_more_than_160_pixels():
    x, y = MR.make_pair((1, 160, 200), "uniform")
    with pytest.raises(ValueError):
        MR.image_metrics(x, y)
    assert math.isnan(MR.image_metrics(x, y, ms_ssim=False)["out"][0, 3])


def _nan(a):
    return np.array([np.nan if v is None else v for v in a], dtype=np.float64)


def test_restatement_equals_the_recorded_values():
    exp = json.load(open(GOLDEN))
    assert exp["seed"] == MR.SEED and sorted(exp["cases"]) == sorted(c[0] for c in MR.cases())
    for name, shape, pair, ms in MR.cases():
        e = exp["cases"][name]
        r = MR.image_metrics(*MR.make_pair(shape, pair), clamp=False, ms_ssim=ms)
        for key, got in (("out", r["out"][0]), ("levels", r["levels"][0]), ("relu_inputs", r["relu_inputs"][0])):
            want = _nan(e[key])
            got = got.ravel()
            assert np.array_equal(np.isnan(got), np.isnan(want)), (name, key)
            ok = ~np.isnan(want)
            assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= 1e-12, (name, key)
        assert abs(r["mse"][0] - e["mse"]) <= 1e-12
        assert 0 < e["dev32"] < 1e-3


def test_recorded_cases_keep_every_relu_input_away_from_zero():
    """The GPU test compares by tolerance; rounding must never decide a relu branch."""
    exp = json.load(open(GOLDEN))
    for name, shape, pair, ms in MR.cases():
        if ms:
            v = _nan(exp["cases"][name]["relu_inputs"])
            assert np.abs(v).min() > 1e-3, (name, v)


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    """Each rejection of riggs_image_metrics happens before any HIP call (the pointers are never dereferenced on the host)."""
    from riggs_amd import _lib
    L = _lib.lib()
    P = 4096  # a non-NULL, aligned stand-in for a device pointer
    big = 1 << 40

    def call(B=1, C=3, H=200, W=200, x=P, y=P, clamp=1, ms=1, out=P, ws=P, n=big):
        return L.riggs_image_metrics(B, C, H, W, x, y, clamp, ms, out, None, ws, n, None)

    def rejected(match, **kw):
        assert call(**kw) != 0
        assert match in L.riggs_last_error(), L.riggs_last_error()

    rejected(b"B and C", B=0)
    rejected(b"B and C", C=0)
    for which in ("x", "y", "out", "ws"):
        rejected(b"NULL", **{which: None})
    need = L.riggs_image_metrics_workspace_floats(1, 3, 200, 200)
    assert need > 0
    rejected(b"workspace", n=need - 1)
    rejected(b"160", H=160, W=400)
    rejected(b"160", H=400, W=160)
    rejected(b"11 x 11", H=10, W=40, ms=0)
    rejected(b"11 x 11", H=40, W=10, ms=0)
    # the workspace grows with the batch and holds the pyramid only where the image admits MS-SSIM
    assert L.riggs_image_metrics_workspace_floats(2, 3, 200, 200) == 2 * need
    assert L.riggs_image_metrics_workspace_floats(1, 3, 160, 160) < L.riggs_image_metrics_workspace_floats(1, 3, 161, 161) // 4


def test_write_numerical_res(tmp_path):
    from riggs_amd.metrics import COLUMNS, write_numerical_res
    assert COLUMNS == ("l1", "psnr", "ssim", "lpips", "ms_ssim", "alex_lpips")
    table = torch.tensor([[0.0123, 31.256, 0.98765, 0.01234, 0.99449, 0.0212],
                          [0.0200, 28.004, 0.91235, float("nan"), 0.95, float("nan")]], dtype=torch.float64)
    means = {"l1": 0.01615, "psnr": 29.63, "ssim": 0.95, "lpips": 0.01234, "ms_ssim": 0.972245, "alex_lpips": float("nan")}
    path = tmp_path / "numerical_res.txt"
    write_numerical_res(str(path), table, means)
    assert path.read_text() == ("ID\tpsnr\tssim\tlpips\tms_ssim\talex_lpips\n"
                                "0\t31.26\t0.9877\t0.0123\t0.9945\t0.0212\n"
                                "1\t28.00\t0.9123\tnan\t0.9500\tnan\n"
                                "mean\t29.63\t0.9500\t0.0123\t0.9722\tnan\n")
