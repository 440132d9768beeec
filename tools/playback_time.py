"""Times the playback of a pose track over one canonical cloud, both ways, in one process:

  a  the per-pose way: ``SkeletonWarp.deform_by_pose`` per pose (with the WeightMLP head on: the head per pose), and — for the
     skinning-weight view — the colours per frame through ``d_values['nn_idx']`` / ``['nn_weight']`` (a second skinning launch
     that writes both) and ``get_color_for_skinning_weights`` (torch ops), as render_rig.py:143-159 does;
  b  ``SkeletonWarp.deform_sequence`` for the whole track plus ``SkeletonWarp.skinning_colors`` once.

Both under ``torch.no_grad()``.  Two sizes: 300 000 Gaussians / 24 joints / 60 poses, and 10 000 Gaussians / 24 joints / 200
poses (ceil(N / 256) = 40 workgroups: the underfilled case, where the track is split over gridDim.y); for K = -1, K = 3 and
K = -1 with the WeightMLP head (fp32, through torch).  A repetition is one whole track; device events around it; 3 warm-up and
11 timed repetitions per variant, the variants alternated; medians.  Also timed on their own: the per-pose loop without the
colours, ``deform_sequence`` alone, ``skinning_colors`` alone.  Writes profiles/playback_times.json (or the path after --out)
with the device's name and the clocks rocm-smi reports before and after.  Fails when no GPU is found."""
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import playback as PB  # noqa: E402
from riggs_amd import synth  # noqa: E402
from riggs_amd.skeleton import SkeletonWarp  # noqa: E402

SIZES = [(300_000, 24, 60), (10_000, 24, 200)]
CONFIGS = [("K=-1", -1, False), ("K=3", 3, False), ("K=-1+WeightMLP", -1, True)]
WARMUP, REPS = 3, 11


def one(N, J, M, K, head):
    sc = synth.make_scene(N, J, 1234)
    torch.manual_seed(0)
    sw = SkeletonWarp(joints=sc["joints"], parent_indices=sc["parents"], K=K, hyper_dim=8, use_skinning_weight_mlp=head,
                      use_template_offsets=False).cuda()
    sw._node_radius.data = sc["node_radius"].cuda()
    x = sc["xyz"].cuda()
    mask = torch.sigmoid(torch.randn(N, 1, generator=torch.Generator().manual_seed(1))).cuda()
    g = torch.Generator().manual_seed(2)
    keys = [{"local_rotation": (torch.tensor([1.0, 0, 0, 0]) + 0.3 * torch.randn(J, 4, generator=g)).cuda(),
             "global_trans": (0.02 * torch.randn(1, 3, generator=g)).cuda()} for _ in range(5)]
    poses = PB.run_interpolation(keys, "cuda", num_frames=M // 4)  # four segments
    lr, gt = poses["local_rotation"], poses["global_trans"]
    assert lr.shape[0] == M
    nodes = sw.nodes.detach()[:, :3]

    def loop(colours):
        last = None
        for f in range(M):
            d = sw.deform_by_pose(x, {"local_rotation": lr[f], "global_trans": gt[f]}, mask)
            last = d["d_xyz"]
            if colours:
                last = PB.get_color_for_skinning_weights(x, d["nn_idx"], d["nn_weight"], nodes)
        return last

    def seq():
        return sw.deform_sequence(x, poses, mask), sw.skinning_colors(x, "blend")

    variants = {"a_loop_with_colours": lambda: loop(True), "b_sequence_and_colours_once": seq, "a_loop_deform_only": lambda: loop(False),
                "b_deform_sequence_only": lambda: sw.deform_sequence(x, poses, mask), "b_skinning_colors_only": lambda: sw.skinning_colors(x)}
    times = {k: [] for k in variants}
    with torch.no_grad():
        for _ in range(WARMUP):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(REPS):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        # the two ways agree
        d = sw.deform_by_pose(x, {"local_rotation": lr[M - 1], "global_trans": gt[M - 1]}, mask)
        s, c = seq()
        ref_c = PB.get_color_for_skinning_weights(x, d["nn_idx"], d["nn_weight"], nodes)
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))  # noqa: E731
        agree = {"d_xyz_last_frame": rel(s["d_xyz"][M - 1], d["d_xyz"]), "d_rotation_last_frame": rel(s["d_rotation"][M - 1], d["d_rotation"]),
                 "colours": rel(c, ref_c)}
    med = {k + "_ms": statistics.median(v) for k, v in times.items()}
    spread = {k + "_min_max_ms": [min(v), max(v)] for k, v in times.items()}
    a, b = med["a_loop_with_colours_ms"], med["b_sequence_and_colours_once_ms"]
    return {"N": N, "J": J, "poses": M, "pass_frames": PB.sequence_pass_frames(J, K), **med, **spread,
            "a_over_b": a / b, "deform_only_a_over_b": med["a_loop_deform_only_ms"] / med["b_deform_sequence_only_ms"],
            "max_err_over_max_b_vs_a": agree}


def clocks():
    """The shader and memory clocks rocm-smi reports for the first card at this moment (a read-only query), or why not."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=10)
        d = json.loads(r.stdout)
        card = d[sorted(d.keys())[0]]
        return {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower()}
    except Exception as e:  # noqa: BLE001
        return {"unavailable": str(e)[:80]}


def main():
    if not torch.cuda.is_available():
        sys.exit("playback_time: no GPU found")
    props = torch.cuda.get_device_properties(0)
    out = {"what": "one pose track over one cloud, ms per track (device events, %d warm-up + %d timed tracks per variant, alternated, "
                   "medians); a: deform_by_pose per pose (+ colours through nn_idx / nn_weight per frame), b: deform_sequence "
                   "(+ skinning_colors once)" % (WARMUP, REPS),
           "device": torch.cuda.get_device_name(0), "compute_units": props.multi_processor_count,
           "clocks_before": clocks(), "results": {}}
    for N, J, M in SIZES:
        for name, K, head in CONFIGS:
            key = "N=%d J=%d poses=%d %s" % (N, J, M, name)
            out["results"][key] = one(N, J, M, K, head)
            print(key, json.dumps(out["results"][key]), flush=True)
    out["clocks_after"] = clocks()
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "playback_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
