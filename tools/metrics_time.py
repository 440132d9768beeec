"""Times the evaluation report (riggs_amd.metrics.image_metrics: L1, PSNR, SSIM, MS-SSIM from one C call) against the same
quantities through the float32 torch-op form of tests/metrics_ref.py on the same GPU — the sequence of ops the reference's
packages issue — at (3, 800, 800) with B = 1 and B = 20 frames, and ``evaluate`` over 20 cameras (one call per chunk of frames)
against the per-frame loop (``chunk=1``: one call per frame, as the reference scores its frames).

Device time by events around a loop of calls after a warm-up; the median of repeated windows.  Launch counts from the
profiler's device-side events in an untimed pass.  Writes profiles/metrics_times.json (or the path after --out); ``--lib PATH``
loads that libriggs_hip.so instead of the tree's (two builds are compared each in a process of its own) and ``--legs image_metrics``
leaves the ``evaluate`` leg out.  Needs the GPU: there is no CPU fallback."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import _lib  # noqa: E402

if "--lib" in sys.argv:
    _lib.SO_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])  # (before the first lib() call)

from riggs_amd import metrics as M  # noqa: E402
from riggs_amd import synth  # noqa: E402
from riggs_amd.gaussian_model import GaussianModel  # noqa: E402
from riggs_amd.render import render  # noqa: E402
from riggs_amd.skeleton import SkeletonModel  # noqa: E402
from tests import metrics_ref as MR  # noqa: E402

C, H, W = 3, 800, 800


def timed(fn, iters, warm=3, windows=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0) / iters)
        dev.append(e0.elapsed_time(e1) / iters)
    return {"device_ms_median": statistics.median(dev), "device_ms_min": min(dev), "device_ms_max": max(dev),
            "wall_ms_median": statistics.median(wall), "calls_per_window": iters, "windows": windows}


def launches(fn):
    """Kernels the device ran for one call (an untimed pass under the profiler)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n if n > 0 else "not measured"
    except Exception as exc:  # (a profiler that does not start says so in the file; the timings do not depend on it)
        return "not measured: %s" % type(exc).__name__


def images(B):
    g = torch.Generator().manual_seed(11 + B)
    smooth = torch.nn.functional.interpolate(torch.rand(B, C, H // 8 + 2, W // 8 + 2, generator=g), size=(H, W), mode="bilinear",
                                             align_corners=True)
    return smooth.cuda().contiguous(), (smooth + 0.08 * torch.randn(B, C, H, W, generator=g)).cuda().contiguous()


def report_legs():
    out = {}
    for B in (1, 20):
        x, y = images(B)
        hip = lambda: M.image_metrics(x, y, clamp=True, ms_ssim=True)  # noqa: E731
        ops = lambda: MR.metrics_torch(x, y, clamp=True, ms_ssim=True, dtype=torch.float32)[0]  # noqa: E731
        diff = (hip().double() - ops().double()).abs().max(0).values.tolist()
        iters = 50 if B == 1 else 10
        out["B=%d" % B] = {"hip": dict(timed(hip, iters), launches=launches(hip)),
                           "torch_ops_float32": dict(timed(ops, iters), launches=launches(ops)),
                           "max_abs_difference_l1_psnr_ssim_msssim": diff}
    return out


def evaluate_leg(n_cams=20, N=100_000, J=24):
    class Pipe:
        convert_SHs_python = compute_cov3D_python = debug = False
    sc = synth.make_scene(N, J, 1234)
    gm = GaussianModel.from_tensors(sc["xyz"], sc["features_dc"], sc["features_rest"], sc["scaling"], sc["rotation"], sc["opacity"],
                                    device="cuda")
    torch.manual_seed(7)
    sk = SkeletonModel(joints=sc["joints"], parent_indices=sc["parents"], K=-1, hyper_dim=8, use_skinning_weight_mlp=False,
                       use_template_offsets=False)
    sk.deform._node_radius.data = sc["node_radius"].cuda()
    bg = torch.zeros(3, device="cuda")
    cams = []
    with torch.no_grad():
        for k in range(n_cams):
            cam = synth.look_at_camera(H, W, azimuth_deg=18.0 * k, fid=0.05 + 0.045 * k).to("cuda")
            d = sk.step(gm.get_xyz.detach(), sk.deform.expand_time(cam.fid + 0.03), motion_mask=gm.motion_mask)
            cam.original_image = render(cam, gm, Pipe, bg, d["d_xyz"], d["d_rotation"], torch.zeros_like(d["d_scaling"]))["render"]
            cams.append(cam)
    batched = lambda: M.evaluate(cams, gm, sk, Pipe, bg, chunk=n_cams)  # noqa: E731
    per_frame = lambda: M.evaluate(cams, gm, sk, Pipe, bg, chunk=1)  # noqa: E731
    # (the LPIPS columns are NaN without callables: compared as zeros)
    diff = torch.nan_to_num(batched()[0] - per_frame()[0]).abs().max(0).values.tolist()
    return {"what": "%d cameras, %d Gaussians, %d joints, %d x %d: deformation + render + metrics per camera; per evaluate() call"
                    % (n_cams, N, J, H, W),
            "chunk=%d" % n_cams: timed(batched, 3, warm=1, windows=5), "chunk=1": timed(per_frame, 3, warm=1, windows=5),
            "max_abs_difference_of_the_two_tables_per_column": diff}


def main():
    assert torch.cuda.is_available(), "metrics_time.py measures on the GPU"
    legs = sys.argv[sys.argv.index("--legs") + 1].split(",") if "--legs" in sys.argv else ["image_metrics", "evaluate"]
    out = {"what": "evaluation report at (%d, %d, %d); per call" % (C, H, W), "device": torch.cuda.get_device_name(0),
           "library": _lib.SO_PATH}
    if "image_metrics" in legs:
        out["image_metrics"] = report_legs()
    if "evaluate" in legs:
        out["evaluate"] = evaluate_leg()
    for k, v in out.items():
        print(k, json.dumps(v))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "metrics_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
