"""Times the stage-1 node regularisers (arap_loss + elastic_loss + acc_loss, forward and backward) on the HIP path against the
same losses in torch ops (tests/node_reg_ref.py's arithmetic in fp32, the rotations by torch.linalg.svd on the device), at
M = 512 and 8192 nodes.  Host time: wall clock per iteration of an eagerly issued loop, synchronised at the end; device time:
CUDA events around the same loop.  Writes profiles/node_reg_times.json (or the path after --out)."""
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import node_reg as NR  # noqa: E402
from tests import node_reg_ref as R  # noqa: E402


def _inputs(M, hyper=8, T_arap=2, T_el=8):
    g = torch.Generator().manual_seed(M)
    nodes = torch.cat([torch.rand(M, 3, generator=g) * 0.05 * M ** (1 / 3), 1e-2 + 0.02 * torch.randn(M, hyper, generator=g)], -1)
    return dict(nodes=nodes.cuda(), radius=(math.log(0.15) + 0.3 * torch.randn(M, generator=g)).cuda(),
                wl=(0.5 * torch.randn(M, 1, generator=g)).cuda(), seq=(nodes[None, :, :3] + 0.01 * torch.randn(T_arap, M, 3, generator=g)).cuda(),
                nt=(nodes[:, None, :3] + 0.01 * torch.randn(M, T_el, 3, generator=g)).cuda(),
                n3=(nodes[:, None, :3] + 0.01 * torch.randn(M, 3, 3, generator=g)).cuda(), hyper=hyper)


def hip_step(d):
    nodes = d["nodes"].requires_grad_(True)
    seq, nt, n3 = (d[k].requires_grad_(True) for k in ("seq", "nt", "n3"))
    idx, _ = NR.connectivity_padded(seq[0].detach(), K=10)
    la = NR.arap_error_padded(seq, idx)
    kidx, _ = NR.node_knn(nodes.detach(), 3)
    w = NR.node_graph_weight(nodes, d["radius"], d["wl"], d["hyper"], kidx)
    le = NR.elastic_energy(nt, kidx[:, 1:].contiguous(), w[:, 1:])
    lc = NR.acc_energy(n3)
    (la + le + lc).backward()


def torch_step(d):
    nodes = d["nodes"].requires_grad_(True)
    seq, nt, n3 = (d[k].requires_grad_(True) for k in ("seq", "nt", "n3"))
    M = nodes.shape[0]
    idx, _ = R.knn_ref(seq[0].detach(), 11, drop_first=True, least_edge_num=3, radius=0.1)
    rows = torch.randint(0, M, (512,), device="cuda") if M > 512 else torch.arange(M, device="cuda")
    with torch.no_grad():
        src = R._edges(seq[0], idx)[rows]
        tgt = R._edges(seq[1], idx)[rows]
        S = src.transpose(1, 2) @ tgt
        U, sig, Vh = torch.linalg.svd(S)
        Rm = Vh.transpose(1, 2) @ U.transpose(1, 2)
    w01 = (idx >= 0)[rows].float()
    r = R._edges(seq[1], idx)[rows] - torch.einsum("sab,snb->sna", Rm, R._edges(seq[0], idx)[rows])
    la = (w01 * (r * r).sum(-1)).sum()
    kidx, _ = R.knn_ref(nodes.detach(), 3)
    w = R.graph_weight_ref(nodes, d["radius"], d["wl"], d["hyper"], kidx)
    le = R.elastic_ref(nt, kidx[:, 1:], w[:, 1:])
    lc = R.acc_ref(n3)
    (la + le + lc).backward()


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


def main():
    out = {"what": "arap (T=2, K=10) + elastic (T=8, K=2, hyper 8) + acc, forward + backward, per iteration", "device": torch.cuda.get_device_name(0)}
    for M in (512, 8192):
        d = _inputs(M)
        out["M%d" % M] = {"hip": timed(hip_step, d), "torch_ops": timed(torch_step, d)}
        print(M, json.dumps(out["M%d" % M]))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "node_reg_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
