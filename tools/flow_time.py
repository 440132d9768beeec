"""Times the optical-flow term of a stage-1 iteration on the HIP path (riggs_amd.render.render_flow, riggs_amd.loss.
optical_flow_loss) against its torch-op form — the reference's formulation over the drop-in rasterizer, tests/flow_ref.py in
float32 on the device: what a user of this library ran before these kernels existed — at the bench scene's size (300 000
Gaussians, 800 x 800, 512 nodes), all legs in one process:

  1. the flow colours, forward + backward (under a seeded cotangent: ``(colours * cot).sum()`` in both forms)
  2. the flow loss, forward + backward
  3. the whole term (node deformation at t2 + render_flow + loss + backward), eagerly issued and replayed from a hipGraph

Device time: events around a loop of iterations after a warm-up; host time: wall clock of issuing the same loop.  The torch-op
form of leg 3 reads the instance count on the host in its rasterizer call (the drop-in rasterizer's contract), so it cannot be
captured; the HIP path keeps the count on the device through a RasterArena.  Writes profiles/flow_times.json (or the path
after --out)."""
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import synth  # noqa: E402
from riggs_amd.control_nodes import ControlNodeWarp  # noqa: E402
from riggs_amd.gaussian_model import GaussianModel  # noqa: E402
from riggs_amd.loss import optical_flow_loss  # noqa: E402
from riggs_amd.node_network import DeformNetwork  # noqa: E402
from riggs_amd.rasterizer import RasterArena  # noqa: E402
from riggs_amd.render import flow_colors, render_flow  # noqa: E402
from tests import flow_ref as FR  # noqa: E402

N, H, W, M, HYPER = 300_000, 800, 800, 512, 8


def scene():
    sc = synth.make_scene(N, 24, 1234)
    gm = GaussianModel.from_tensors(sc["xyz"], sc["features_dc"], sc["features_rest"], sc["scaling"], sc["rotation"], sc["opacity"],
                                    device="cuda")
    g = torch.Generator().manual_seed(5)
    gm.fea_dim, gm.with_motion_mask = HYPER + 1, True
    gm.feature = torch.nn.Parameter(torch.cat([0.02 * torch.randn(N, HYPER, generator=g), 2.0 + torch.randn(N, 1, generator=g)], -1).cuda())
    cam1 = synth.look_at_camera(H, W, fid=0.3).to("cuda")
    cam2 = synth.look_at_camera(H, W, azimuth_deg=47.0, elevation_deg=19.0, fid=0.35).to("cuda")
    torch.manual_seed(7)
    net = DeformNetwork(is_blender=True, local_frame=False).cuda()
    cn = ControlNodeWarp(node_num=M, K=3, local_frame=False, d_rot_as_res=True, hyper_dim=HYPER, network=net, is_blender=True).cuda()
    sel = torch.randperm(N, generator=g)[:M].cuda()
    with torch.no_grad():
        cn.nodes.copy_(torch.cat([gm.get_xyz.detach()[sel], gm.feature.detach()[sel, :HYPER]], -1))
        cn._node_radius.fill_(math.log(0.2))
    d = dict(gm=gm, cam1=cam1, cam2=cam2, cn=cn,
             d1=(0.01 * torch.randn(N, 3, generator=g)).cuda().requires_grad_(True),
             d2=(0.01 * torch.randn(N, 3, generator=g)).cuda().requires_grad_(True),
             cot=torch.randn(N, 3, generator=g).cuda(),
             image=torch.rand(3, H, W, generator=g).cuda(), gt=torch.rand(3, H, W, generator=g).cuda(),
             motion=(0.05 * torch.randn(3, H, W, generator=g)).cuda().requires_grad_(True),
             alpha=(0.5 + 0.5 * torch.rand(1, H, W, generator=g)).cuda(), flow=(4.0 * torch.randn(H, W, 2, generator=g)).cuda(),
             masks=(torch.rand(H, W, 3, generator=g) > 0.3).float().cuda(),
             fid1=torch.tensor([0.3], device="cuda"), fid2=torch.tensor([0.35], device="cuda"), arena=RasterArena())
    return d


def _zero(d):
    for t in [d["d1"], d["d2"], d["motion"], d["gm"].feature] + list(d["cn"].parameters()) + d["gm"].parameters():
        t.grad = None


def colours_hip(d):
    _zero(d)
    (flow_colors(d["gm"], d["cam1"], d["cam2"], d["d1"], d["d2"]) * d["cot"]).sum().backward()


def colours_torch(d):
    _zero(d)
    gm = d["gm"]
    col = FR.colours(gm._xyz, d["d1"], d["d2"], d["cam1"].full_proj_transform, d["cam2"].full_proj_transform, gm.motion_mask)
    (col * d["cot"]).sum().backward()


def loss_hip(d):
    _zero(d)
    optical_flow_loss(d["image"], d["gt"], d["motion"], d["alpha"], d["flow"], d["masks"], d["fid1"], d["fid2"]).backward()


def loss_torch(d):
    _zero(d)
    FR.flow_loss(d["image"], d["gt"], d["motion"], d["alpha"], d["flow"], d["masks"], d["fid1"], d["fid2"]).backward()


def term_hip(d):
    _zero(d)
    gm = d["gm"]
    d2 = d["cn"](gm.get_xyz.detach(), d["fid2"].reshape(()), gm.feature, gm.motion_mask)["d_xyz"]
    pkg = render_flow(gm, d["cam1"], d["cam2"], d["d1"], d2, 0.0, 0.0, arena=d["arena"])
    optical_flow_loss(d["image"], d["gt"], pkg["render"], pkg["alpha"], d["flow"], d["masks"], d["fid1"], d["fid2"]).backward()


def term_torch(d):
    _zero(d)
    gm = d["gm"]
    d2 = d["cn"](gm.get_xyz.detach(), d["fid2"].reshape(()), gm.feature, gm.motion_mask)["d_xyz"]
    pkg = FR.render_flow_composed(gm, d["cam1"], d["cam2"], d["d1"], d2, 0.0, 0.0)
    FR.flow_loss(d["image"], d["gt"], pkg["render"], pkg["alpha"], d["flow"], d["masks"], d["fid1"], d["fid2"]).backward()


def timed(fn, d, iters=20, warm=3):
    for _ in range(warm):
        fn(d)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn(d)
    e1.record()
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_wall = time.perf_counter() - t0
    return {"host_issue_ms": 1e3 * t_issue / iters, "wall_ms": 1e3 * t_wall / iters, "device_ms": e0.elapsed_time(e1) / iters}


def captured(fn, d, iters=20):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn(d)
            torch.cuda.current_stream().synchronize()
            d["arena"].resolve()
        d["arena"].top_up()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            fn(d)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(iters):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        t_wall = time.perf_counter() - t0
        overflow = int(d["arena"].static_counters.tolist()[1])
    torch.cuda.current_stream().wait_stream(s)
    return {"wall_ms": 1e3 * t_wall / iters, "device_ms": e0.elapsed_time(e1) / iters, "arena_overflow": overflow}


def main():
    d = scene()
    out = {"what": "optical-flow term, N = %d Gaussians, %d x %d, %d nodes; per iteration" % (N, H, W, M),
           "device": torch.cuda.get_device_name(0)}
    out["colours_fwd_bwd"] = {"hip": timed(colours_hip, d), "torch_ops": timed(colours_torch, d)}
    out["loss_fwd_bwd"] = {"hip": timed(loss_hip, d), "torch_ops": timed(loss_torch, d)}
    out["whole_term_eager"] = {"hip": timed(term_hip, d, iters=10), "torch_ops": timed(term_torch, d, iters=10)}
    out["whole_term_captured"] = {"hip": captured(term_hip, d), "torch_ops": "not capturable: the drop-in rasterizer reads the instance count on the host"}
    for k, v in out.items():
        print(k, json.dumps(v))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "flow_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
