"""Fixtures of the node network from the reference's DeformNetwork (imported through _ref_shim, never copied; CPU only).

  node_mlp_w64_params.npz   W = 64 (not is_blender, local_frame, pred_opacity): the reference's own initialisation with biases
                            and head weights redrawn at N(0, 0.05); every parameter (float32)
  node_mlp_w64_grads.npz    inputs, cotangents, float64 outputs, hidden and EVERY parameter gradient of that network
  node_mlp_w256_{a,b,c}.npz W = 256, parameters from tests/node_mlp_ref.integer_params (not stored): R = 200 rows with repeated
                            and distinct times; outputs in full, hidden for the first 50 rows, gradients in full for the small
                            tensors and rows SUBROWS of the wide matrices
  node_mlp_state_dict_layout.json   keys and shapes of DeformNetwork.state_dict() per configuration, and the network.* part of
                            ControlNodeWarp(...).state_dict()
Every npz also records the reference's own float32 run against its float64 run: the largest output deviation (of the tensor's
maximum) and the number of ReLU units whose sign differs.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shim as S  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import node_mlp_ref as NR  # noqa: E402

SUBROWS = [0, 37, 101, 255]
SMALL = 8192
SEEDS = {"a": 31, "b": 118, "c": 119}    # chosen so that the reference's own float32 run flips at most 2e-6 of the ReLU units


def run(net, x, t, cot, dtype):
    net = net.to(dtype)
    pres = []
    hooks = [m.register_forward_hook(lambda mod, i, o: pres.append(o.detach().clone())) for m in net.linear]
    if net.is_blender:
        hooks.append(net.timenet[0].register_forward_hook(lambda mod, i, o: pres.append(o.detach().clone())))
    net.zero_grad()
    out = net(x.to(dtype), t.to(dtype))
    loss = sum((out[k] * cot[k].to(dtype)).sum() for k in NR.OUT_KEYS if out.get(k) is not None)
    loss.backward()
    for h in hooks:
        h.remove()
    g = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    return {k: (v.detach().clone() if torch.is_tensor(v) else None) for k, v in out.items()}, g, pres


def fixture(name, cfg, net, R, seed, store_params):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(R, 3, generator=g) * 2 - 1).float()
    t = torch.rand(R, 1, generator=g).float()
    t[: R // 4] = t[0]                     # repeated times in front, distinct ones behind
    heads = [k for k in NR.OUT_KEYS if not (k == "local_rotation" and not cfg["local_frame"])
             and not (k == "d_opacity" and not cfg["pred_opacity"])]
    width = dict(d_xyz=3, d_scaling=3, d_rotation=4, local_rotation=4, d_opacity=1)
    cot = {k: torch.randn(R, width[k], generator=g).float() for k in heads}
    sd32 = {k: v.detach().clone().float() for k, v in net.state_dict().items()}
    o64, g64, p64 = run(net, x, t, cot, torch.float64)
    net.load_state_dict(sd32)
    o32, g32, p32 = run(net, x, t, cot, torch.float32)
    net.load_state_dict(sd32)
    flips = int(sum(((a > 0) != (b > 0)).sum() for a, b in zip(p64, p32)))
    units = int(sum(a.numel() for a in p64))
    dev = max(float((o32[k].double() - o64[k]).abs().max() / o64[k].abs().max()) for k in heads)
    gdev = max(float((g32[k].double() - g64[k]).abs().max() / max(float(g64[k].abs().max()), 1e-300)) for k in g64)
    z = dict(x=x.numpy(), t=t.numpy(), ref_fp32_mask_flips=np.int64(flips), ref_relu_units=np.int64(units),
             ref_fp32_out_dev=np.float64(dev), ref_fp32_grad_dev=np.float64(gdev))
    for k in heads:
        z["cot/" + k] = cot[k].numpy()
        z["out/" + k] = o64[k].numpy()
    z["out/hidden"] = o64["hidden"][:50].numpy()
    for k, v in g64.items():
        if store_params or v.numel() <= SMALL:
            z["grad/" + k] = v.numpy()
        else:
            z["gradrows/" + k] = v[SUBROWS].numpy()
    if store_params:
        np.savez(os.path.join(HERE, name + "_params.npz"), **{k: v.numpy() for k, v in sd32.items()})
        np.savez(os.path.join(HERE, name + "_grads.npz"), **z)
    else:
        np.savez(os.path.join(HERE, name + ".npz"), **z)
    print(name, "fp32 ref: out dev %.2e grad dev %.2e mask flips %d of %d" % (dev, gdev, flips, units))


def ref_kwargs(cfg):
    return dict(D=8, W=cfg["W"], is_blender=cfg["is_blender"], local_frame=cfg["local_frame"], pred_opacity=cfg["pred_opacity"],
                max_d_scale=cfg["max_d_scale"])


def main():
    S.install()
    with S.quiet():
        from utils.time_utils import ControlNodeWarp, DeformNetwork
    layout = {}
    for key, cfg in NR.CONFIGS.items():
        torch.manual_seed(100)
        net = DeformNetwork(**ref_kwargs(cfg))
        layout[key] = {k: list(v.shape) for k, v in net.state_dict().items()}
        if key == "w64":
            g = torch.Generator().manual_seed(7)
            with torch.no_grad():
                for k, p in net.named_parameters():
                    if k.endswith(".bias") or k.split(".")[0] in dict(NR.HEADS):
                        p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            fixture("node_mlp_w64", cfg, net, 96, 11, True)
        else:
            net.load_state_dict(NR.integer_params(cfg, torch.float32))
            fixture("node_mlp_w256_" + key, cfg, net, 200, SEEDS[key], False)
    with S.quiet():
        cn = ControlNodeWarp(is_blender=True, node_num=16, K=3, hyper_dim=8, local_frame=True)
    layout["control_node_warp_network"] = {k: list(v.shape) for k, v in cn.state_dict().items() if k.startswith("network.")}
    with open(os.path.join(HERE, "node_mlp_state_dict_layout.json"), "w") as f:
        json.dump(layout, f, indent=1)


if __name__ == "__main__":
    main()
