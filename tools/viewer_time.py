"""Times the editor's display step (riggs_amd.viewer.display_frame with its overlay builders) at 800 x 800 against a torch + NumPy
restatement of what the reference does per displayed frame (interactive_GUI.py:127-247, :611-654): the resize on the device, the
device-to-host copy of the frame, the projected points copied to the host, one Python loop iteration per primitive through
the oracle rasteriser of tests/viewer_ref.py (over each primitive's bounding box) STANDING IN FOR OpenCV, and the NumPy blend.
OpenCV is not installed where this runs and its scan conversion is compiled code, so the ``raster`` part of the host path (the
per-primitive loop: each primitive's record and its pixels) says what this stand-in costs, not what ``cv2.polylines`` costs; the
parts are therefore reported one by one, and ``host_without_raster`` (resize + copies + projection + blend) is the part of the
reference's step that does not depend on the stand-in.

Two legs: the skeleton overlay (24 joints: 23 bones and 24 discs) and the trajectory overlay (512 tracks x 32 samples: 15 872
segments).  The HIP path is timed with and without the one device-to-host copy of the finished buffer that the editor makes.
Device time by events around a loop of calls after a warm-up, the median of repeated windows; wall time around the same loop
ending in a synchronise.  Launch counts from the profiler's device-side events in an untimed pass.  Writes
profiles/viewer_times.json (or the path after --out).  Needs the GPU: there is no CPU fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import synth  # noqa: E402
from riggs_amd import viewer as V  # noqa: E402
from tests import viewer_ref as VR  # noqa: E402

H = W = 800


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
            "wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall), "calls_per_window": iters,
            "windows": windows}


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


def host_step(image, points_to_uv, uv_to_table, full_proj, parts):
    """The reference's step for one overlay; ``parts`` accumulates the wall time of each part (seconds)."""
    def lap(name, t0):
        torch.cuda.synchronize()
        parts[name] = parts.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()
    t = time.perf_counter()
    buf = torch.nn.functional.interpolate(image.unsqueeze(0), size=(H, W), mode="bilinear", align_corners=False).squeeze(0)
    buf = buf.permute(1, 2, 0).contiguous().clamp(0, 1).contiguous().detach().cpu().numpy()
    t = lap("resize_and_frame_d2h", t)
    uv = points_to_uv(full_proj)                            # projection on the device, the points copied to the host
    t = lap("projection_and_points_d2h", t)
    table = uv_to_table(uv)                                 # one loop iteration per primitive: its record ...
    rgb, a = VR.paint(table, H, W, boxed=True)              # ... and its pixels
    t = lap("raster", t)
    out = buf * (1 - a[..., None]) + rgb * a[..., None]
    lap("blend", t)
    return out


def editor_uv(points, full_proj):
    hom = torch.cat([points, torch.ones_like(points[..., :1])], dim=-1) @ full_proj
    uv = hom[..., :2] / hom[..., -1:]
    return (uv + 1) / 2 * torch.tensor([H, W], device=points.device)


def leg(name, image, cam, hip_table, host_uv, host_table, host_iters):
    full_proj = cam.full_proj_transform
    buf = torch.empty(H, W, 3, device="cuda")

    def hip():
        return V.display_frame({"render": image}, "render", (H, W), overlays=[hip_table()], out_buffer=buf)

    def hip_d2h():
        return hip().cpu()
    want = host_step(image, host_uv, host_table, full_proj, {})
    got = hip_d2h().double().numpy()
    differing = int((np.abs(got - want).max(-1) > 1e-5).sum())
    parts = {}
    for _ in range(3):
        host_step(image, host_uv, host_table, full_proj, {})
    t0 = time.perf_counter()
    for _ in range(host_iters):
        host_step(image, host_uv, host_table, full_proj, parts)
    host_ms = 1e3 * (time.perf_counter() - t0) / host_iters
    parts = {k: 1e3 * v / host_iters for k, v in parts.items()}
    return {"primitives": int(hip_table().shape[0]),
            "hip": dict(timed(hip, 200), launches=launches(hip)),
            "hip_with_frame_d2h": timed(hip_d2h, 100),
            "host_restatement": {"wall_ms": host_ms, "parts_wall_ms": parts, "host_without_raster_wall_ms": host_ms - parts["raster"],
                                 "iterations": host_iters, "raster": "tests/viewer_ref.py paint(boxed=True), a Python stand-in for OpenCV"},
            "pixels_differing_by_more_than_1e-5": differing}


def main():
    assert torch.cuda.is_available(), "viewer_time.py measures on the GPU"
    out = {"what": "display_frame at %d x %d (render mode, source %d x %d) with one overlay; per displayed frame" % (H, W, H, W),
           "device": torch.cuda.get_device_name(0)}
    g = torch.Generator().manual_seed(5)
    image = torch.rand(3, H, W, generator=g).cuda()
    cam = synth.look_at_camera(H, W, radius=3.2).to("cuda")

    joints, parents = synth.make_skeleton(g, 24)
    d_nodes = (joints + 0.02 * torch.randn(24, 3, generator=g)).cuda()
    colors = V.get_geometric_color(d_nodes)
    par = parents.to("cuda", torch.int32)
    colors_host, parents_host = colors.double().cpu().numpy(), parents.numpy()

    out["skeleton_24_joints"] = leg("skeleton", image, cam, lambda: V.skeleton_overlay(cam, d_nodes, par, node_colors=colors),
                                    lambda full_proj: editor_uv(d_nodes, full_proj).detach().cpu().numpy(),
                                    lambda uv: VR.skeleton_table(uv, np.ones(24, bool), parents_host, colors_host), host_iters=20)

    N = 100_000
    cloud = 0.45 * torch.randn(N, 3, generator=g)
    drift = 0.004 * torch.randn(N, 3, generator=g)
    traj = V.TrajectoryOverlay(gs_num=512, samp_num=32, thickness=1)
    for k in range(40):
        traj.push((cloud + k * drift + 0.002 * torch.randn(N, 3, generator=g)).cuda(), start=torch.tensor([0]))
    jet = V.jet_colors(512)

    def trajectory_uv(full_proj):
        S, head = traj.samples()
        return editor_uv(torch.roll(traj.ring, -head, 0)[:S], full_proj).detach().cpu().numpy()
    out["trajectories_512x32"] = leg("trajectories", image, cam, lambda: traj.primitives(cam), trajectory_uv,
                                     lambda uv: VR.polyline_table(uv, np.ones(uv.shape[:2], bool), jet), host_iters=3)

    for k, v in out.items():
        print(k, json.dumps(v))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "viewer_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
