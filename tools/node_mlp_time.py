"""Time the node network (riggs_amd/node_network.py, three launches per call) against the torch restatement of
tests/node_mlp_ref.py in fp32 on the same GPU, in one process, alternating: forward + backward at the row counts of a stage-1
iteration, the four calls of a node-rendering iteration together, 65 536 rows, and one whole stage-1 iteration both ways.
Writes profiles/node_mlp_times.json (--out PATH): host issue time, wall time and device time (events) per iteration, the median
over the rounds with the smallest and largest round beside it."""
import json
import os
import sys
import time
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import node_mlp_ref as NR  # noqa: E402

WIDTH = dict(d_xyz=3, d_scaling=3, d_rotation=4, local_rotation=4)
CFG = NR.CONFIGS["a"]  # the shipped recipe: is_blender, local_frame, W = 256


def _nets():
    from riggs_amd.node_network import DeformNetwork
    params = NR.integer_params(CFG)
    net = DeformNetwork(is_blender=True, local_frame=True)
    net.load_state_dict({k: v.float() for k, v in params.items()})
    ref = NR.RefNetwork(CFG, OrderedDict((k, v.float()) for k, v in params.items()))
    return net.cuda(), ref.cuda()


def _inputs(rows, seed=0):
    g = torch.Generator().manual_seed(seed)
    calls = []
    for R in rows:
        x = (torch.rand(R, 3, generator=g) * 2 - 1).cuda()
        t = torch.rand(R, 1, generator=g).cuda()
        cot = {k: torch.randn(R, w, generator=g).cuda() for k, w in WIDTH.items()}
        calls.append((x, t, cot))
    return calls


def step(net, calls):
    for p in net.parameters():
        p.grad = None
    for x, t, cot in calls:
        out = net(x, t)
        sum((out[k] * cot[k]).sum() for k in cot).backward()


def one_round(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_wall = time.perf_counter() - t0
    return (1e3 * t_issue / iters, 1e3 * t_wall / iters, e0.elapsed_time(e1) / iters)


def alternate(fns, iters=20, rounds=5, warm=3):
    """fns: name -> callable.  `rounds` rounds of `iters` timed iterations each, the variants alternating round by round."""
    for f in fns.values():
        for _ in range(warm):
            f()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(one_round(f, iters))
    out = {}
    for k, rs in got.items():
        out[k] = {}
        for i, name in enumerate(("host_issue_ms", "wall_ms", "device_ms")):
            v = sorted(r[i] for r in rs)
            out[k][name] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
    return out


def stage1_iteration():
    from tests.test_gpu_node_mlp import _Rec, _module, _stage1, _stage1_loss, _stage1_warp
    cfg, params, gm, cam, nodes, weight = _stage1()
    target = torch.rand(3, 96, 96, generator=torch.Generator().manual_seed(9)).cuda()
    tt = torch.tensor(0.4, device="cuda")
    native = _module(cfg, params)
    native.keep_stored_activations = False
    ref = NR.RefNetwork(cfg, OrderedDict((k, v.float().cuda()) for k, v in params.items()))
    fns = {}
    for name, net in (("native", native), ("torch_restatement", ref)):
        cn = _stage1_warp(net, nodes, weight)

        def f(cn=cn):
            for p in cn.parameters():
                p.grad = None
            _stage1_loss(cn, gm, cam, target, 3000, tt).backward()
        fns[name] = f
    return alternate(fns, iters=10, rounds=5)


def main():
    out = {"what": "DeformNetwork (is_blender, local_frame, W = 256, D = 8) forward + backward per iteration: the HIP node "
                   "network against the torch restatement in fp32, alternating rounds in one process; ms",
           "device": torch.cuda.get_device_name(0), "rounds": 5, "iters_per_round": 20}
    net, ref = _nets()
    for label, rows in (("R512", [512]), ("R1024", [1024]), ("R1536", [1536]), ("R4096", [4096]), ("R8192", [8192]),
                        ("four_calls_2000_4096_1536_1024", [2000, 4096, 1536, 1024]), ("R65536", [65536])):
        calls = _inputs(rows)
        iters = 20 if rows[0] < 65536 else 5
        out[label] = alternate({"native": lambda: step(net, calls), "torch_restatement": lambda: step(ref, calls)}, iters=iters)
        print(label, json.dumps(out[label]))
    out["stage1_iteration_M512_N6000_96x96"] = stage1_iteration()
    print("stage1", json.dumps(out["stage1_iteration_M512_N6000_96x96"]))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "node_mlp_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
