"""Times the motion-mask term of a stage-1 iteration (train_gui.py:1123-1130) at the bench scene's size (300 000 Gaussians, 24
joints, 800 x 800, the ``synth`` scene, with a motion mask), both ways, in one process:

  A  the second ``render(render_motion=True, detach...)`` through the general path in an arena of its own (preprocess, depth
     sort, tile sort, compositing; a backward that computes every geometry gradient and drops it), forward plus the backward
     of ``motion_mask_loss``;
  B  ``render(..., lists=main.lists)``: the recolour pass over the main frame's tile lists (csrc/recolor.hip), forward plus the
     same backward.

Device events around every repetition; 20 warm-up and 200 timed repetitions per variant, the variants alternated (A, B, A) so
that A is measured twice and its own spread is known.  Writes the medians, A's spread, the instance count R and the B-against-A
image and gradient differences to profiles/recolor_times.json (or the path after --out).  Fails when no GPU is found."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import synth  # noqa: E402
from riggs_amd.gaussian_model import GaussianModel  # noqa: E402
from riggs_amd.loss import motion_mask_loss  # noqa: E402
from riggs_amd.rasterizer import RasterArena  # noqa: E402
from riggs_amd.render import render  # noqa: E402

N, J, H, W, HYPER = 300_000, 24, 800, 800, 8
WARMUP, REPS = 20, 200
MOTION = dict(render_motion=True, detach_xyz=True, detach_rot=True, detach_scale=True, detach_opacity=True)


class Pipe:
    convert_SHs_python = compute_cov3D_python = debug = False


def main():
    if not torch.cuda.is_available():
        sys.exit("recolor_time: no GPU found")
    sc = synth.make_scene(N, J, 1234)
    gm = GaussianModel.from_tensors(sc["xyz"], sc["features_dc"], sc["features_rest"], sc["scaling"], sc["rotation"], sc["opacity"],
                                    device="cuda")
    g = torch.Generator().manual_seed(5)
    gm.fea_dim, gm.with_motion_mask = HYPER + 1, True
    gm.feature = torch.nn.Parameter(torch.cat([0.02 * torch.randn(N, HYPER, generator=g), torch.randn(N, 1, generator=g)], -1).cuda())
    cam = synth.look_at_camera(H, W, fid=0.3).to("cuda")
    bg = torch.zeros(3, device="cuda")
    gt = (torch.rand(1, H, W, generator=g) > 0.5).float().cuda()
    d = (0.0, 0.0, 0.0)
    arena = RasterArena()
    render(cam, gm, Pipe, bg, *d, arena=arena)
    main_pkg = render(cam, gm, Pipe, bg, *d, arena=arena, keep_lists=True)  # the frame's main render, outside the timed region
    R = int(main_pkg.lists.counters[0].item()) & 0xFFFFFFFF

    def variant(lists):
        gm.feature.grad = None
        pkg = render(cam, gm, Pipe, bg, *d, lists=lists, **MOTION)
        motion_mask_loss(gt, pkg["render"][0]).backward()
        return pkg["render"].detach(), gm.feature.grad[:, -1]

    variants = {"A": lambda: variant(None), "B": lambda: variant(main_pkg.lists), "A_again": lambda: variant(None)}
    for _ in range(WARMUP):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    for _ in range(REPS):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            wall[k].append(1e3 * (time.perf_counter() - t0))
            times[k].append(e0.elapsed_time(e1))
    img_a, grad_a = (t.clone() for t in variants["A"]())
    img_b, grad_b = (t.clone() for t in variants["B"]())
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))  # noqa: E731
    frac = lambda a, b, r: float(((a - b).abs() > r * b.abs().max()).float().mean())  # noqa: E731
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"what": "motion-mask term (second render + motion_mask_loss, forward + backward), N = %d Gaussians, %d joints, %d x %d; "
                   "ms per repetition, device events, %d warm-up + %d timed repetitions per variant, alternated" % (N, J, H, W, WARMUP, REPS),
           "device": torch.cuda.get_device_name(0), "instances_R": R,
           "A_second_render_ms": med["A"], "A_again_ms": med["A_again"], "A_spread_ms": abs(med["A"] - med["A_again"]),
           "B_lists_ms": med["B"],
           "wall_ms": {k: statistics.median(v) for k, v in wall.items()},
           "B_vs_A": {"image_max_err_over_max": rel(img_b, img_a), "image_frac_beyond_1e-5": frac(img_b, img_a, 1e-5),
                      "grad_max_err_over_max": rel(grad_b, grad_a), "grad_frac_beyond_2e-5": frac(grad_b, grad_a, 2e-5)},
           "B_faster_than_A_by_more_than_its_spread": bool(med["B"] < min(med["A"], med["A_again"]) - abs(med["A"] - med["A_again"]))}
    for k, v in out.items():
        print(k, json.dumps(v))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "recolor_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    if not out["B_faster_than_A_by_more_than_its_spread"]:
        sys.exit("recolor_time: B is not faster than A by more than A's spread")


if __name__ == "__main__":
    main()
