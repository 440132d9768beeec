"""Times the fused image loss (riggs_amd.loss.l1_ssim: L1 + SSIM forward, then the backward to the rendered image) at
(3, 800, 800), as tools/metrics_time.py times the evaluation report: device time by events around a loop of forward + backward
calls after a warm-up; the median and the spread of repeated windows.  A call at this size is bound by the host (two autograd
nodes, ~50 us of kernels), so the launches are also timed by the library's own event timers (``loss_fwd`` = forward + finish
kernel, ``loss_bwd``), windows of the same length.

``--lib PATH`` loads that libriggs_hip.so instead of the tree's (two builds are compared each in a process of its own);
``--out FILE`` is where the result goes (default profiles/loss_times.json).  Needs the GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import _lib  # noqa: E402

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


def kernel_us(fn, iters, windows=7):
    """Mean device time per launch scope from the library's event timers, one figure per window."""
    import ctypes
    lib = _lib.lib()
    rows = {"loss_fwd": [], "loss_bwd": []}
    tot, cnt = ctypes.c_float(), ctypes.c_int32()
    for _ in range(windows):
        lib.riggs_prof_reset()
        lib.riggs_prof_enable(0xFFFFFFFF)
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        lib.riggs_prof_enable(0)
        for i in range(lib.riggs_prof_count()):
            name = lib.riggs_prof_name(i).decode()
            if name in rows:
                _lib.check(lib.riggs_prof_read(i, ctypes.byref(tot), ctypes.byref(cnt)), "riggs_prof_read")
                rows[name].append(1e3 * tot.value / max(cnt.value, 1))
    return {k: {"us_median": statistics.median(v), "us_min": min(v), "us_max": max(v), "launches_per_window": iters,
                "windows": windows} for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", help="the libriggs_hip.so to load instead of the tree's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_times.json"))
    args = ap.parse_args()
    if args.lib:
        _lib.SO_PATH = os.path.abspath(args.lib)  # (before the first lib() call)
    assert torch.cuda.is_available(), "loss_time.py measures on the GPU"
    from riggs_amd.loss import l1_ssim
    g = torch.Generator().manual_seed(0)
    x = torch.rand(C, H, W, generator=g).cuda().requires_grad_(True)
    y = torch.rand(C, H, W, generator=g).cuda()

    def step():
        l1, s = l1_ssim(x, y)
        (0.8 * l1 + 0.2 * (1 - s)).backward()
        x.grad = None

    out = {"what": "l1_ssim forward + backward at (%d, %d, %d); per call" % (C, H, W), "device": torch.cuda.get_device_name(0),
           "library": _lib.SO_PATH, "l1_ssim_fwd_bwd": timed(step, 50), "kernels": kernel_us(step, 50)}
    for k, v in out.items():
        print(k, json.dumps(v))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
