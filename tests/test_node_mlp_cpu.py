"""CPU: the node network's restatement against the reference's float64 fixtures, the module's parameter layout against the
recorded one, and the C ABI's symbols."""
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import node_mlp_ref as NR

FIXTURES = ("w64", "a", "b", "c")
SUBROWS = [0, 37, 101, 255]


def load_fixture(golden_dir, key, dtype=torch.float64):
    cfg = NR.CONFIGS[key]
    if key == "w64":
        z = np.load(os.path.join(golden_dir, "node_mlp_w64_grads.npz"))
        pz = np.load(os.path.join(golden_dir, "node_mlp_w64_params.npz"))
        params = OrderedDict((k, torch.from_numpy(pz[k]).to(dtype)) for k in NR.param_shapes(cfg))
    else:
        z = np.load(os.path.join(golden_dir, "node_mlp_w256_%s.npz" % key))
        params = NR.integer_params(cfg, dtype)
    return cfg, params, z


def fixture_cot(z):
    return {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("cot/")}


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def compare_grads(got, z, bound, record=None):
    """got: name -> tensor; every stored gradient (full, or rows SUBROWS) within bound of its tensor's maximum."""
    n = 0
    for k in z.files:
        if k.startswith("grad/"):
            e = rel_err(got[k[5:]].detach().cpu().numpy(), z[k])
        elif k.startswith("gradrows/"):
            e = rel_err(got[k[9:]].detach().cpu().numpy()[SUBROWS], z[k])
        else:
            continue
        n += 1
        if record is not None:
            record(k, e)
        assert e <= bound, "%s: %.3g beyond %.1e of the maximum" % (k, e, bound)
    assert n >= 20


@pytest.mark.parametrize("key", FIXTURES)
def test_restatement_reproduces_the_reference_in_float64(golden_dir, key):
    cfg, params, z = load_fixture(golden_dir, key)
    assert list(params.keys()) == list(NR.param_shapes(cfg).keys())
    out, g = NR.grads(params, torch.from_numpy(z["x"]), torch.from_numpy(z["t"]), cfg, fixture_cot(z))
    for k in z.files:
        if k.startswith("out/"):
            mine = out[k[4:]].detach().numpy()
            mine = mine[:50] if k == "out/hidden" else mine
            assert rel_err(mine, z[k]) <= 1e-10, k
    compare_grads(g, z, 1e-10)
    # the fixture seeds were chosen so that the reference's own float32 run stays within the mask cap of the issue
    assert int(z["ref_fp32_mask_flips"]) <= 2e-6 * int(z["ref_relu_units"])
    assert float(z["ref_fp32_out_dev"]) < 1e-5


def test_pinned_masks_reproduce_the_free_run():
    cfg = NR.CONFIGS["w64"]
    params = NR.integer_params(cfg)
    g = torch.Generator().manual_seed(0)
    x, t = torch.rand(9, 3, generator=g, dtype=torch.float64), torch.rand(9, 1, generator=g, dtype=torch.float64)
    cot = {"d_xyz": torch.randn(9, 3, generator=g), "d_rotation": torch.randn(9, 4, generator=g)}
    out, g0 = NR.grads(params, x, t, cfg, cot)
    masks = {"act": torch.stack([(a > 0) for a in out["act"]]).double(), "timenet": None}
    out1, g1 = NR.grads(params, x, t, cfg, cot, masks=masks)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def _layout(golden_dir):
    with open(os.path.join(golden_dir, "node_mlp_state_dict_layout.json")) as f:
        return json.load(f)


def _module(cfg):
    from riggs_amd.node_network import DeformNetwork
    return DeformNetwork(D=8, W=cfg["W"], is_blender=cfg["is_blender"], local_frame=cfg["local_frame"],
                         pred_opacity=cfg["pred_opacity"], max_d_scale=cfg["max_d_scale"])


@pytest.mark.parametrize("key", FIXTURES)
def test_module_has_the_reference_layout_and_initialisers(golden_dir, key):
    cfg = NR.CONFIGS[key]
    net = _module(cfg)
    sd = net.state_dict()
    want = _layout(golden_dir)[key]
    assert [(k, list(v.shape)) for k, v in sd.items()] == [(k, v) for k, v in want.items()]
    assert list(want.keys()) == list(NR.param_shapes(cfg).keys())
    for k, v in sd.items():
        head = k.split(".")[0]
        if k.endswith(".bias") and head != "timenet":
            assert float(v.abs().max()) == 0.0, k
    std = {"gaussian_warp": 1e-5, "gaussian_scaling": 1e-8, "gaussian_rotation": 1e-5, "local_rotation": 1e-4, "gaussian_opacity": 1e-5}
    for name, s in std.items():
        if name + ".weight" in sd:
            got = float(sd[name + ".weight"].std())
            assert 0.5 * s < got < 2.0 * s, (name, got)
    bound = (6.0 / sd["linear.1.weight"].shape[1]) ** 0.5
    assert 0.9 * bound < float(sd["linear.1.weight"].abs().max()) <= bound
    assert net.name == "mlp" and net.reg_loss == 0.
    grp = net.trainable_parameters()
    assert len(grp) == 1 and grp[0]["name"] == "mlp" and len(grp[0]["params"]) == len(want)
    net.update(100)
    assert net.t_multires == (6 if cfg["is_blender"] else 10)


def test_unsupported_flags_raise():
    from riggs_amd.node_network import DeformNetwork
    for kw in (dict(pred_color=True), dict(pred_color=True, resnet_color=False, hash_color=True),
               dict(pred_color=True, resnet_color=False), dict(progressive_brand_time=True)):
        with pytest.raises(NotImplementedError):
            DeformNetwork(**kw)
    with pytest.raises(NotImplementedError):
        DeformNetwork(W=96)
    with pytest.raises(NotImplementedError):
        DeformNetwork(D=6)


def test_control_node_warp_exposes_and_loads_the_network_keys(golden_dir):
    from riggs_amd.control_nodes import ControlNodeWarp
    from riggs_amd.node_network import DeformNetwork
    want = _layout(golden_dir)["control_node_warp_network"]
    cn = ControlNodeWarp(node_num=16, K=3, hyper_dim=8, local_frame=True, is_blender=True,
                         network=DeformNetwork(is_blender=True, local_frame=True))
    sd = cn.state_dict()
    mine = OrderedDict((k, list(v.shape)) for k, v in sd.items() if k.startswith("network."))
    assert list(mine.items()) == list(want.items())
    new = {k: (torch.full_like(v, 0.25) if k.startswith("network.") else v) for k, v in sd.items()}
    cn.load_state_dict(new)
    assert float(cn.network.linear[5].weight.detach().min()) == 0.25 and float(cn.network.timenet[2].bias.detach().max()) == 0.25
    names = [g["name"] for g in cn.trainable_parameters()]
    assert "deform" in names


def test_header_declares_and_library_exports_the_node_mlp_entries():
    from riggs_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "riggs_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(riggs_node_mlp_[a-z0-9_]+)\s*\(", txt)))
    assert declared == ["riggs_node_mlp_acts_floats", "riggs_node_mlp_backward", "riggs_node_mlp_backward_workspace_floats",
                        "riggs_node_mlp_forward", "riggs_node_mlp_hidden_offset"]
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name) and name in _lib.exported_symbols()
    # sizes, and rejection of what the kernels do not support (no GPU needed: validation precedes every HIP call)
    assert L.riggs_node_mlp_acts_floats(512, 256, 8) >= 512 * (8 * 256 + 93 + 256)
    assert L.riggs_node_mlp_backward_workspace_floats(512, 256, 8) >= 512 * 8 * 256
    off = L.riggs_node_mlp_hidden_offset(512, 256, 8)
    assert off + 512 * 256 == L.riggs_node_mlp_acts_floats(512, 256, 8)
    for (r, w, d) in ((0, 256, 8), (65537, 256, 8), (512, 96, 8), (512, 256, 6)):
        assert L.riggs_node_mlp_acts_floats(r, w, d) == 0
    import ctypes as C
    net = _lib.NodeMlp()
    for (r, w, d) in ((0, 256, 8), (65537, 256, 8), (512, 96, 8), (512, 512, 8), (512, 256, 4)):
        net.width, net.depth = w, d
        rc = L.riggs_node_mlp_forward(C.byref(net), r, *([None] * 2), 1, *([None] * 7))
        assert rc != 0 and b"riggs_node_mlp" in L.riggs_last_error()
    net.width, net.depth = 256, 8
    assert L.riggs_node_mlp_forward(C.byref(net), 16, *([None] * 2), 1, *([None] * 7)) != 0   # null parameters
