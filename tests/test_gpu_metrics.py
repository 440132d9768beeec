"""GPU: the evaluation report (riggs_amd.metrics, csrc/metrics.hip) against the float64 restatement of its definitions
(tests/metrics_ref.py, recorded in tests/golden/metrics_expected.json and checked against the restatement on the CPU by
tests/test_metrics_cpu.py).

Tolerance of the SSIM quantities: both the float32 torch-op form and the kernels evaluate the cancelling ``E[x^2] - mu^2`` in
float32, so per case the HIP result may deviate from the float64 value by 4x what the float32 form deviates (``dev32`` of the
recorded file; the margin covers another summation order and contraction in an equally precise evaluation), at least 1e-6.
l1 and the mean squared error: 1e-6 relative (float32 differences and squares, float64 sums); psnr: 1e-4 dB.  What the HIP path
showed is written to profiles/metrics_parity.json when RIGGS_WRITE_PROFILES=1 is set (the committed record is made that way)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = json.load(open(os.path.join(ROOT, "tests", "golden", "metrics_expected.json")))["cases"]
SHOWN = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_record():
    yield
    if SHOWN and os.environ.get("RIGGS_WRITE_PROFILES") == "1":
        out = os.path.join(ROOT, "profiles")
        with open(os.path.join(out, "metrics_parity.json"), "w") as f:
            json.dump({"largest_ssim_deviation": max(v["ssim_dev"] for v in SHOWN.values()),
                       "largest_deviation_over_tolerance": max(v["ssim_dev"] / v["tolerance"] for v in SHOWN.values()),
                       "cases": SHOWN}, f, indent=1)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(a):
    return np.array([np.nan if v is None else v for v in a], dtype=np.float64)


@pytest.mark.parametrize("name,shape,pair,ms", MR.cases(), ids=[c[0] for c in MR.cases()])
def test_parity_with_the_float64_restatement(name, shape, pair, ms):
    from riggs_amd import metrics as M
    e = EXPECTED[name]
    x, y = MR.make_pair(shape, pair)
    out, levels = M.image_metrics(_dev(x), _dev(y), clamp=False, ms_ssim=ms, return_levels=True)
    out, levels = out.double().cpu().numpy()[0], levels.double().cpu().numpy()[0].ravel()
    want, want_levels = _nan(e["out"]), _nan(e["levels"])
    tol = MR.tolerance(e["dev32"])
    if ms:  # rounding must not decide a relu branch in a case compared by tolerance
        assert np.abs(_nan(e["relu_inputs"])).min() > 1e-3
    l1_rel = abs(out[0] / want[0] - 1)
    mse_rel = abs(10 ** (-out[1] / 10) / e["mse"] - 1)
    psnr_err = abs(out[1] - want[1])
    assert np.array_equal(np.isnan(levels), np.isnan(want_levels))
    ok = ~np.isnan(want_levels)
    devs = [np.abs(levels[ok] - want_levels[ok]).max(), abs(out[2] - want[2])]
    if ms and pair != "negative":
        devs.append(abs(out[3] - want[3]))
    SHOWN[name] = {"ssim_dev": float(max(devs)), "dev32": e["dev32"], "tolerance": tol, "l1_rel": float(l1_rel),
                   "mse_rel": float(mse_rel), "psnr_err_db": float(psnr_err)}
    print(name, SHOWN[name])
    assert l1_rel <= 1e-6 and mse_rel <= 1e-6 and psnr_err <= 1e-4
    assert max(devs) <= tol
    if ms:
        assert (out[3] == 0.0 and out[2] < 0) if pair == "negative" else out[3] > 0
    else:
        assert math.isnan(out[3])


def _stack(shape, scale=None):
    xs, ys = zip(*(MR.make_pair(shape, p) for p in MR.PAIRS))
    x, y = np.concatenate(xs), np.concatenate(ys)
    if scale is not None:
        x, y = np.float32(x * 1.4 - 0.2), np.float32(y * 1.4 - 0.2)
    return _dev(x), _dev(y)


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.parametrize("shape,ms", [((3, 385, 390), True), ((1, 75, 43), False)])
def test_clamp_on_load_equals_clamped_inputs(shape, ms):
    from riggs_amd import metrics as M
    x, y = _stack(shape, scale=True)
    assert float(x.min()) < 0 and float(x.max()) > 1
    a = M.image_metrics(x, y, clamp=True, ms_ssim=ms, return_levels=True)
    b = M.image_metrics(x.clamp(0.0, 1.0), y.clamp(0.0, 1.0), clamp=False, ms_ssim=ms, return_levels=True)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    c = M.image_metrics(x, y, clamp=False, ms_ssim=ms)
    assert not _same(a[0], c)


@pytest.mark.parametrize("shape,ms", [((3, 385, 390), True), ((3, 176, 163), True), ((2, 43, 12), False)])
def test_a_frames_row_does_not_depend_on_the_batch_or_the_run(shape, ms):
    from riggs_amd import metrics as M
    x, y = _stack(shape)
    both = M.image_metrics(x, y, clamp=False, ms_ssim=ms, return_levels=True)
    again = M.image_metrics(x, y, clamp=False, ms_ssim=ms, return_levels=True)
    assert _same(both[0], again[0]) and _same(both[1], again[1])
    for b in range(3):
        one = M.image_metrics(x[b:b + 1], y[b:b + 1], clamp=False, ms_ssim=ms, return_levels=True)
        assert _same(one[0], both[0][b:b + 1]) and _same(one[1], both[1][b:b + 1])
    swapped = M.image_metrics(x.flip(0), y.flip(0), clamp=False, ms_ssim=ms)
    assert _same(swapped.flip(0), both[0])


def test_thin_wrappers_return_the_columns():
    from riggs_amd import metrics as M
    x, y = _stack((3, 176, 163))
    t = M.image_metrics(x, y, clamp=False)
    assert M.psnr(x, y).shape == (3, 1) and torch.equal(M.psnr(x, y)[:, 0], t[:, 1])
    assert torch.equal(M.ssim(x, y, data_range=1., reduction="none"), t[:, 2])
    assert torch.equal(M.ssim(x, y), t[:, 2].mean())
    assert torch.equal(M.ssim(x[0], y[0]), t[0, 2])
    assert torch.equal(M.ms_ssim(x, y, data_range=1., size_average=False), t[:, 3])
    assert torch.equal(M.ms_ssim(x, y), t[:, 3].mean())
    assert torch.equal(M.ssim(x * 2, y * 2, data_range=2.0, reduction="none"), M.ssim((x * 2) / 2.0, (y * 2) / 2.0, reduction="none"))
    with pytest.raises(NotImplementedError):
        M.ssim(x, y, kernel_size=7)
    with pytest.raises(NotImplementedError):
        M.ssim(x, y, reduction="sum")
    with pytest.raises(NotImplementedError):
        M.ms_ssim(x, y, win_size=7)


def test_identical_images_and_refusals():
    from riggs_amd import _lib as L
    from riggs_amd import metrics as M
    x, _ = _stack((3, 176, 163))
    t = M.image_metrics(x, x).cpu()
    assert bool((t[:, 0] == 0).all()) and bool(torch.isinf(t[:, 1]).all()) and bool((t[:, 1] > 0).all())
    assert float((t[:, 2:] - 1).abs().max()) <= 1e-6
    small = x[:, :, :160]
    with pytest.raises(ValueError):
        M.image_metrics(small, small)
    assert bool(torch.isnan(M.image_metrics(small, small, ms_ssim=False)[:, 3]).all())
    with pytest.raises(L.RiggsHipError):
        M.image_metrics(x.cpu(), x.cpu())
    with pytest.raises(L.RiggsHipError):
        M.image_metrics(x[:, :, :10], x[:, :, :10], ms_ssim=False)


def test_evaluate_on_a_synthetic_scene(tmp_path):
    from riggs_amd import metrics as M
    from riggs_amd import synth
    from riggs_amd.gaussian_model import GaussianModel
    from riggs_amd.render import render
    from riggs_amd.skeleton import SkeletonModel

    class Pipe:
        convert_SHs_python = compute_cov3D_python = debug = False
    H, W = 192, 176
    sc = synth.make_scene(2000, 6, 1241, scale=0.03)
    gm = GaussianModel.from_tensors(sc["xyz"], sc["features_dc"], sc["features_rest"], sc["scaling"], sc["rotation"], sc["opacity"])
    torch.manual_seed(5)
    sk = SkeletonModel(joints=sc["joints"], parent_indices=sc["parents"], K=-1, hyper_dim=8, use_skinning_weight_mlp=False,
                       use_template_offsets=False)
    sk.deform._node_radius.data = sc["node_radius"].cuda()
    bg = torch.zeros(3, device="cuda")

    def frame(cam, fid):
        with torch.no_grad():
            d = sk.step(gm.get_xyz.detach(), sk.deform.expand_time(fid), motion_mask=gm.motion_mask)
            d_rot = torch.zeros_like(d["d_rotation"]) if gm.use_isotropic_gs else d["d_rotation"]
            return render(cam, gm, Pipe, bg, d["d_xyz"], d_rot, torch.zeros_like(d["d_scaling"]), d_opacity=d.get("d_opacity"),
                          d_color=d.get("d_color"))["render"]
    cams = []
    for k in range(5):
        cam = synth.look_at_camera(H, W, azimuth_deg=30.0 + 60.0 * k, fid=0.2 + 0.1 * k).to("cuda")
        cam.original_image = frame(cam, cam.fid + 0.05)   # ground truth: the same scene at a perturbed time
        cams.append(cam)
    table, means = M.evaluate(cams, gm, sk, Pipe, bg, chunk=2)
    assert table.shape == (5, 6) and table.dtype == torch.float64 and not table.is_cuda
    rows = torch.cat([M.image_metrics(frame(c, c.fid).clamp(0.0, 1.0)[None], c.original_image.clamp(0.0, 1.0)[None], clamp=False)
                      for c in cams]).double().cpu()
    assert torch.equal(table[:, [0, 1, 2, 4]], rows)
    assert bool(torch.isnan(table[:, [3, 5]]).all()) and math.isnan(means["lpips"]) and math.isnan(means["alex_lpips"])
    assert bool((table[:, 0] > 0).all()) and bool((table[:, 2] < 1).all()) and bool((table[:, 4] < 1).all())  # (not a trivial scene)
    for i, k in enumerate(M.COLUMNS):
        if k not in ("lpips", "alex_lpips"):
            assert abs(means[k] - float(np.mean(table[:, i].numpy()))) <= 1e-6
    seen = []

    def fake_lpips(a, b):
        assert a.shape == b.shape == (1, 3, H, W) and float(a.min()) >= 0 and float(a.max()) <= 1
        seen.append(float((a - b).abs().mean()))
        return (a - b).abs().mean().reshape(1, 1, 1, 1)
    table2, means2 = M.evaluate(cams, gm, sk, Pipe, bg, lpips_fn=fake_lpips, chunk=8)
    assert torch.equal(table2[:, [0, 1, 2, 4]], rows) and bool(torch.isnan(table2[:, 5]).all())
    assert np.abs(table2[:, 3].numpy() - np.float32(seen)).max() <= 1e-7 and abs(means2["lpips"] - np.mean(seen)) <= 1e-6
    # cameras of another size go into a chunk of their own
    odd = synth.look_at_camera(H + 8, W, fid=0.3).to("cuda")
    odd.original_image = frame(odd, odd.fid + 0.05)
    table3, _ = M.evaluate(cams[:3] + [odd] + cams[3:], gm, sk, Pipe, bg, chunk=4)
    assert torch.equal(table3[[0, 1, 2, 4, 5]][:, [0, 1, 2, 4]], rows)
    # the report file parses back to the table at its printed precision
    path = tmp_path / "numerical_res.txt"
    M.write_numerical_res(str(path), table2, means2)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == ["ID", "psnr", "ssim", "lpips", "ms_ssim", "alex_lpips"] and len(lines) == 7
    for i, line in enumerate(lines[1:6]):
        f = line.split("\t")
        assert int(f[0]) == i
        for v, col, prec in zip(f[1:5], (1, 2, 3, 4), (2, 4, 4, 4)):
            assert abs(float(v) - float(table2[i, col])) <= 0.5 * 10 ** -prec + 1e-9
        assert f[5] == "nan"
    f = lines[6].split("\t")
    assert f[0] == "mean" and abs(float(f[1]) - means2["psnr"]) <= 0.005 + 1e-9 and abs(float(f[4]) - means2["ms_ssim"]) <= 5e-5 + 1e-9
