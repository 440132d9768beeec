"""Times farthest-point sampling on the HIP path (csrc/fps.hip: one launch per picked point) against the torch loop it replaces
(riggs_amd.gaussian_model.farthest_point_sample_torch: about eight launches per point) on the same device, at the sizes the
library samples at: 300 000 -> 512 (node initialisation), 300 000 -> 5 000 (sampling_and_prune) and 1 024 -> 200 (the skeleton
extraction) over 3-vectors, and 300 000 x 48 -> 1 024 and 20 000 x 48 -> 512 (the stage-1 node sampling over trajectories of
16 times) over wide rows.  Device time: events around one whole sweep, the median of ``--repeats`` sweeps per side, the two sides alternating;
the host's issue time of a sweep next to it.  Also counts the picks on which the two agree (the torch loop's argmax leaves ties
undefined on the device and its sum may round differently: informational).  Writes profiles/fps_times.json (or the path after
--out)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd.fps import farthest_point_sample, farthest_point_sample_rows  # noqa: E402
from riggs_amd.gaussian_model import farthest_point_sample_torch as fps_torch  # noqa: E402

CASES = ((300000, 3, 512), (300000, 3, 5000), (1024, 3, 200), (300000, 48, 1024), (20000, 48, 512))  # rows, width, picks


def once(fn, x, npoint, start):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn(x, npoint, start=start)
    e1.record()
    issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), 1e3 * issue, out


def main():
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 7
    out = {"what": "farthest-point sampling, one whole sweep; device ms = median of %d sweeps, sides alternating" % repeats,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for N, D, npoint in CASES:
        fps_hip = farthest_point_sample if D == 3 else farthest_point_sample_rows
        g = torch.Generator().manual_seed(N + npoint)
        x = torch.randn(1, N, D, generator=g).cuda()
        start = torch.tensor([N // 3], device="cuda")
        for fn in (fps_hip, fps_torch):  # warm-up: code objects, the allocator
            once(fn, x, min(npoint, 64), start)
        t = {"hip": [], "torch_loop": []}
        h = {"hip": [], "torch_loop": []}
        for _ in range(repeats):
            for name, fn in (("hip", fps_hip), ("torch_loop", fps_torch)):
                ms, issue, idx = once(fn, x, npoint, start)
                t[name].append(ms)
                h[name].append(issue)
                if name == "hip":
                    a = idx
                else:
                    same = int((a == idx).sum())
        from riggs_amd import _lib as L
        row = {"blocks": int(L.lib().riggs_fps_blocks(N)) if D == 3 else None, "picks_equal": same, "bytes_read_per_launch": 4 * N * (D + 1),
               "hip": {"device_ms": statistics.median(t["hip"]), "min_ms": min(t["hip"]), "max_ms": max(t["hip"]),
                       "host_issue_ms": statistics.median(h["hip"]), "us_per_pick": 1e3 * statistics.median(t["hip"]) / npoint},
               "torch_loop": {"device_ms": statistics.median(t["torch_loop"]), "min_ms": min(t["torch_loop"]), "max_ms": max(t["torch_loop"]),
                              "host_issue_ms": statistics.median(h["torch_loop"]),
                              "us_per_pick": 1e3 * statistics.median(t["torch_loop"]) / npoint}}
        row["torch_over_hip"] = row["torch_loop"]["device_ms"] / row["hip"]["device_ms"]
        out["cases"]["n%d_p%d" % (N, npoint) if D == 3 else "n%d_d%d_p%d" % (N, D, npoint)] = row
        print(N, D, npoint, json.dumps(row))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fps_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
