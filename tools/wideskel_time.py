"""Times of the deformation path over skeleton sizes on both sides of the 64-joint switch (J <= 64: one-wave chain, LDS records
of <= 63 bones; J > 64: the workgroup chain, the 256-joint instantiation of the skinning forward and the bone-lane
backward in passes of 64 bones), trees and chains, N = 300 k:
FK forward / backward, the all-bones skinning forward / backward (incl. its finish kernel) — each from a graph of 20 launches,
best of 5 replays — and the PoseMLP forward / backward (the network SkeletonWarp builds, eager calls, mean of 20).
usage: python tools/wideskel_time.py [--out profiles/wideskel_times.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import synth  # noqa: E402
from riggs_amd.skeleton import PoseMLP, fk_forward  # noqa: E402


def graph_us(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    best = 1e9
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / reps * 1e6)
    return best


def case(N, J, chain):
    sc = synth.make_scene(N, J, 11, chain=chain)
    lib = L.lib()
    x = sc["xyz"].cuda()
    joints, par = sc["joints"].cuda(), sc["parents"].to(torch.int32).cuda()
    rho = sc["node_radius"].cuda()
    gt = sc["global_trans"].reshape(-1).cuda()
    q = sc["local_rotation"].cuda().contiguous()
    mask = sc["motion_mask"].reshape(-1).contiguous().cuda()
    tr, nrot, dn = fk_forward(q, joints, par, gt)
    dG, gn, dq, dgt = torch.randn(J, 12, device="cuda"), torch.randn(J, 3, device="cuda"), torch.empty(J, 4, device="cuda"), torch.zeros(3, device="cuda")
    d_xyz, d_rot = torch.empty(N, 3, device="cuda"), torch.empty(N, 4, device="cuda")
    g_xyz, g_rot = torch.randn(N, 3, device="cuda"), torch.randn(N, 4, device="cuda")
    bdG, bdrho, bdgt, bdmask = torch.empty(J, 12, device="cuda"), torch.empty(J, device="cuda"), torch.empty(3, device="cuda"), torch.empty(N, device="cuda")
    ws = torch.empty(int(lib.riggs_lbs_backward_workspace_bytes(N, J)), dtype=torch.uint8, device="cuda")
    st = lambda: L.stream_ptr()  # noqa: E731
    r = {"N": N, "J": J, "chain": chain}
    dep = [0] * J
    for i in range(1, J):
        dep[i] = dep[int(sc["parents"][i])] + 1
    r["depth"] = max(dep)
    r["fk_fwd_us"] = graph_us(lambda: lib.riggs_fk_forward(J, q.data_ptr(), joints.data_ptr(), par.data_ptr(), gt.data_ptr(), tr.data_ptr(),
                                                           nrot.data_ptr(), dn.data_ptr(), st()))
    r["fk_bwd_us"] = graph_us(lambda: lib.riggs_fk_backward(J, q.data_ptr(), joints.data_ptr(), par.data_ptr(), dG.data_ptr(), gn.data_ptr(),
                                                            dq.data_ptr(), dgt.data_ptr(), st()))
    r["lbs_fwd_us"] = graph_us(lambda: lib.riggs_lbs_forward(N, J, -1, x.data_ptr(), joints.data_ptr(), par.data_ptr(), rho.data_ptr(),
                                                             tr.data_ptr(), nrot.data_ptr(), gt.data_ptr(), mask.data_ptr(), None,
                                                             d_xyz.data_ptr(), d_rot.data_ptr(), None, None, None, st()))
    r["lbs_bwd_us"] = graph_us(lambda: lib.riggs_lbs_backward(N, J, -1, x.data_ptr(), joints.data_ptr(), par.data_ptr(), rho.data_ptr(),
                                                              tr.data_ptr(), nrot.data_ptr(), gt.data_ptr(), mask.data_ptr(), None,
                                                              g_xyz.data_ptr(), g_rot.data_ptr(), bdG.data_ptr(), bdrho.data_ptr(),
                                                              bdgt.data_ptr(), bdmask.data_ptr(), None, ws.data_ptr(), st()))
    B = J - 1
    r["lbs_fwd_ns_per_pair"] = r["lbs_fwd_us"] * 1e3 / (N * B)
    r["lbs_bwd_ns_per_pair"] = r["lbs_bwd_us"] * 1e3 / (N * B)
    torch.manual_seed(0)
    net = PoseMLP(1, 4 * J).cuda()
    t = torch.tensor([0.37], device="cuda")
    for _ in range(3):
        out = net(t)
        (out["rotation"].sum() + out["translation"].sum()).backward()
    torch.cuda.synchronize()
    fwd = bwd = 0.0
    for _ in range(20):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        out = net(t)
        e1.record()
        (out["rotation"].sum() + out["translation"].sum()).backward()
        e2.record()
        torch.cuda.synchronize()
        fwd += e0.elapsed_time(e1) * 1e3 / 20
        bwd += e1.elapsed_time(e2) * 1e3 / 20
    r["pose_mlp_fwd_us"], r["pose_mlp_bwd_us"] = fwd, bwd
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wideskel_times.json"))
    ap.add_argument("--N", type=int, default=300_000)
    a = ap.parse_args()
    rows = [case(a.N, J, chain) for J in (24, 64, 65, 128, 200, 256) for chain in (False, True)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, open(a.out, "w"), indent=1)
