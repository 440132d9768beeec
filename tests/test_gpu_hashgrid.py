"""GPU: the hash-grid encoding (csrc/hashgrid.hip) against the NumPy restatement of the published algorithm
(tests/hashgrid_ref.py), and riggs_amd.hash_network.HashDeformNetwork against what the reference's module computes around that
oracle (tests/golden/make_hashgrid_golden.py).  The table gradient is a sum by float atomics: its last bits depend on the arrival
order, so everything here compares within a tolerance, never bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from tests import hashgrid_ref as HR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# dense and hashed levels, and heavy collisions within a row and across rows (1 024 entries per hashed level) / cell counts that are
# no multiple of 8
CONFIGS = {"L12-base2": dict(n_levels=12, n_features_per_level=2, log2_hashmap_size=10, base_resolution=2, per_level_scale=2.0),
           "L5-base3": dict(n_levels=5, n_features_per_level=2, log2_hashmap_size=10, base_resolution=3, per_level_scale=1.5)}
_CASES = {}


def _case(cfg_name, D, R, masked):
    """Inputs and the oracle's answers, computed once per case and left unchanged."""
    key = (cfg_name, D, R, masked)
    if key not in _CASES:
        cfg = CONFIGS[cfg_name]
        rng = np.random.default_rng(1000 * D + R + (7 if masked else 0) + len(cfg_name))
        total = HR.level_table(D, **cfg)[1]
        LF = 2 * cfg["n_levels"]
        x = (rng.random((R, D)) * 1.7 - 0.3).astype(np.float32)
        # the first rows: one row that mixes the four special coordinates, then every coordinate at 0, at 1, at -0.2, at 1.3
        special = np.array([[0.0, 1.0, -0.2, 1.3], [0.0] * 4, [1.0] * 4, [-0.2] * 4, [1.3] * 4], dtype=np.float32)[:, :D]
        if D == 3:
            special[0] = [1.3, 0.0, -0.2]
        x[:min(R, 5)] = special[:min(R, 5)]
        table = (rng.random((total, 2)) * 2 - 1).astype(np.float32)
        g = rng.standard_normal((R, LF)).astype(np.float32)
        mask = None
        if masked:
            mask = rng.random(LF).astype(np.float32)
            mask[[1, 4, 5, LF - 2, LF - 1]] = 0.0          # one column of level 0, both of level 2 and of the last level
        out, g_table, g_abs = HR.encode(x, table, D, cfg, mask=mask, g_out=g)
        for a in (x, table, g, out, g_table, g_abs):
            a.setflags(write=False)
        _CASES[key] = dict(cfg=cfg, x=x, table=table, g=g, mask=mask, out=out, g_table=g_table, g_abs=g_abs)
    return _CASES[key]


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("R", [1, 63, 65, 257])
@pytest.mark.parametrize("D", [3, 4])
@pytest.mark.parametrize("cfg_name", list(CONFIGS))
def test_encoding_forward_and_table_gradient_against_the_oracle(cfg_name, D, R, masked):
    """Forward within 1e-5 max|table| (a float32 sum of at most 16 weighted terms is off by about 1.2e-6 of it at the most);
    table gradient within 1e-5 sum |w mask g| per entry, exactly zero where nothing (or only masked columns) arrives."""
    from riggs_amd.hash_network import HashGridEncoding
    c = _case(cfg_name, D, R, masked)
    enc = HashGridEncoding(D, c["cfg"])
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(np.array(c["table"])).reshape(-1))
    mask = None if c["mask"] is None else torch.from_numpy(np.array(c["mask"])).cuda()
    out = enc(torch.from_numpy(np.array(c["x"])).cuda(), mask)
    assert out.shape == (R, 2 * c["cfg"]["n_levels"]) and out.dtype is torch.float32
    err = np.abs(out.detach().cpu().numpy().astype(np.float64) - c["out"]).max()
    tol = 1e-5 * float(np.abs(c["table"]).max())
    print("forward: max error %.3e, tolerance %.3e" % (err, tol))
    out.backward(torch.from_numpy(np.array(c["g"])).cuda())
    got = enc.params.grad.cpu().numpy().astype(np.float64).reshape(-1, 2)
    gerr = np.abs(got - c["g_table"])
    worst = float((gerr / np.maximum(c["g_abs"], 1e-300)).max())
    print("table gradient: worst error %.3e of sum |w mask g| (tolerance 1e-5), %d of %d values touched"
          % (worst, int((c["g_abs"] > 0).sum()), got.size))
    assert err <= tol
    assert (gerr <= 1e-5 * c["g_abs"]).all()
    assert not got[c["g_abs"] == 0].any()
    if masked:
        assert not out[:, [1, 4, 5]].any()


def _golden_net(name):
    from riggs_amd.hash_network import HashDeformNetwork
    z = np.load(os.path.join(GOLDEN, "hashgrid_net_%s.npz" % name))
    net = HashDeformNetwork(hidden_dim=64, hash_time=name == "xyzt", local_frame=True, pred_opacity=True, bbox=z["bbox"].tolist())
    sd = {k[len("param/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}
    n = net.hashgrid.encoding.params.numel()
    table = HR.table_values(n, int(z["table_a"]), int(z["table_b"]), int(z["table_m"])) * np.float32(z["table_scale"])
    sd["hashgrid.encoding.params"] = torch.from_numpy(table)
    net.load_state_dict(sd)            # strict: the golden's names are this module's names
    return net, z


@pytest.mark.parametrize("name", ["xyz", "xyzt"])
def test_network_against_the_reference_golden(name):
    """Outputs, the gradients of the trunk's first layer and of the table against the reference's HashDeformNetwork run in
    float32 on the CPU around the oracle encoding.  Tolerance: 10 x the deviation of that float32 run from its float64 rerun
    (make_hashgrid_golden.py measures it on the same encoding input; recorded as ref_fp32_out_dev / ref_fp32_grad_dev), relative
    to each tensor's largest magnitude: outputs 10 x 8.21e-7 (xyz) / 10 x 3.62e-7 (xyzt), gradients 10 x 3.99e-7 / 10 x 2.76e-7."""
    net, z = _golden_net(name)
    net.update(3250)
    assert np.abs(net.hashgrid.mask.cpu().numpy() - z["mask_3250"]).max() < 1e-6
    x, t = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["t"]).cuda()
    enc_in = net.contract(x)
    enc_in = torch.cat([enc_in, t], -1) if name == "xyzt" else enc_in
    assert np.array_equal(enc_in.cpu().numpy(), z["enc_input"])      # the contraction gives the CPU's bits
    out = net(x, t)
    assert set(out) == {"d_xyz", "d_rotation", "d_scaling", "d_opacity", "d_color", "local_rotation"} and out["d_color"] is None
    keys = ["d_xyz", "d_rotation", "d_scaling", "d_opacity", "local_rotation"]
    otol, gtol = 10 * float(z["ref_fp32_out_dev"]), 10 * float(z["ref_fp32_grad_dev"])
    sum((out[k] * torch.from_numpy(z["cot/" + k]).cuda()).sum() for k in keys).backward()
    fails = []
    for k in keys:
        want = z["out/" + k]
        err = np.abs(out[k].detach().cpu().numpy() - want).max() / np.abs(want).max()
        print("%s %s: %.3e of the largest magnitude (tolerance %.3e)" % (name, k, err, otol))
        fails += [(k, err)] if not err <= otol else []
    grads = {"mlp.layers.0.weight": net.mlp.layers[0].weight.grad, "mlp.layers.0.bias": net.mlp.layers[0].bias.grad}
    for k, g in grads.items():
        want = z["grad/" + k]
        err = np.abs(g.cpu().numpy() - want).max() / np.abs(want).max()
        print("%s grad %s: %.3e (tolerance %.3e)" % (name, k, err, gtol))
        fails += [(k, err)] if not err <= gtol else []
    gt = net.hashgrid.encoding.params.grad.cpu().numpy()
    idx, scale = z["grad_table_index"].astype(np.int64), float(z["grad_table_max"])
    err = np.abs(gt[idx] - z["grad_table_value"]).max() / scale
    rest = gt.copy()
    rest[idx] = 0
    print("%s table gradient: %.3e at the %d touched values, %.3e elsewhere (tolerance %.3e)" % (name, err, idx.size, np.abs(rest).max() / scale, gtol))
    fails += [("table", err)] if not err <= gtol else []
    fails += [("untouched table", np.abs(rest).max() / scale)] if not np.abs(rest).max() / scale <= gtol else []
    assert not fails, fails


def test_state_dict_round_trip_and_the_reference_s_names():
    from riggs_amd.hash_network import HashDeformNetwork
    layout = json.load(open(os.path.join(GOLDEN, "hashgrid_state_dict_layout.json")))
    for key, hash_time in (("no_hash_time", False), ("hash_time", True)):
        a = HashDeformNetwork(hash_time=hash_time, local_frame=True, pred_opacity=True)
        a.update(2500)
        sd = a.state_dict()
        assert {k: list(v.shape) for k, v in sd.items()} == layout[key] and all(v.is_cuda for v in sd.values())
        b = HashDeformNetwork(hash_time=hash_time, local_frame=True, pred_opacity=True)
        b.load_state_dict(sd)
        assert int(b.hashgrid.current_step) == 2500
        b.update(int(b.hashgrid.current_step))     # the mask is no part of a checkpoint: the trainer's update() restores it
        x, t = torch.rand(65, 3, device="cuda") * 3 - 1.5, torch.rand(65, 1, device="cuda")
        oa, ob = a(x, t), b(x, t)
        assert all(torch.equal(oa[k], ob[k]) for k in oa if oa[k] is not None)
        # a dict with the recorded names and shapes, as a checkpoint written by the reference holds it (CPU tensors)
        g = torch.Generator().manual_seed(3)
        ref_sd = {k: (torch.rand(s, generator=g) - 0.5 if k != "hashgrid.current_step" else torch.tensor(4000, dtype=torch.int32))
                  for k, s in layout[key].items()}
        ref_sd["bbox"] = torch.tensor([-1.0, 1.5])
        b.load_state_dict(ref_sd)
        assert int(b.hashgrid.current_step) == 4000 and b.bbox.tolist() == [-1.0, 1.5]
        assert torch.equal(b.hashgrid.encoding.params.detach().cpu(), ref_sd["hashgrid.encoding.params"])
        assert all(torch.isfinite(v).all() for v in b(x, t).values() if v is not None)


def test_control_node_warp_with_the_hash_network():
    from riggs_amd.control_nodes import ControlNodeWarp
    from riggs_amd.hash_network import HashDeformNetwork
    g = torch.Generator().manual_seed(21)
    N, M, H = 3000, 64, 2
    pcl = (torch.rand(N, 3, generator=g) * torch.tensor([2.0, 1.0, 3.0]) - torch.tensor([0.5, 0.2, 1.9])).cuda()
    net = HashDeformNetwork(hidden_dim=64, local_frame=True)
    cn = ControlNodeWarp(node_num=M, K=3, local_frame=True, hyper_dim=H, use_hash=True, network=net).cuda()
    assert cn.use_hash and net.bbox.tolist() == [-2.0, 2.0]
    cn.init(None, pcl, start=0)
    want = torch.stack([pcl.min() - .1, pcl.max() + .1])
    assert torch.equal(net.bbox, want) and net.bbox.dtype is torch.float32 and "network.bbox" in cn.state_dict()
    cn.init(None, pcl * 2, force_init=True, reset_bbox=False, start=0)
    assert torch.equal(net.bbox, want)
    cn.init(None, pcl, force_init=True, start=0)
    with torch.no_grad():                       # (the reference draws the trunk's last layer at 1e-5: lift it so that gradients are not denormal)
        net.mlp.layers[-1].weight.normal_(0, 0.1)
        net.hashgrid.encoding.params.uniform_(-0.5, 0.5)
    mask0 = net.hashgrid.mask.clone()
    cn.update(3250)
    assert not torch.equal(net.hashgrid.mask, mask0) and int(net.hashgrid.current_step) == 3250
    assert np.abs(net.hashgrid.mask.cpu().numpy() - HR.cosine_mask(3250)).max() < 1e-6
    feature = torch.nn.Parameter(torch.cat([0.02 * torch.randn(N, H, generator=g), 2.0 + torch.randn(N, 1, generator=g)], -1).cuda())
    dv = cn(pcl, torch.tensor(0.3, device="cuda"), feature, torch.sigmoid(feature[:, -1:]), iteration=3250)
    cot = {k: torch.randn(dv[k].shape, generator=g).cuda() for k in ("d_xyz", "d_rotation", "d_scaling")}
    sum((dv[k] * cot[k]).sum() for k in cot).backward()
    gt = net.hashgrid.encoding.params.grad
    assert gt is not None and torch.isfinite(gt).all() and gt.abs().max() > 0
    assert torch.isfinite(cn.nodes.grad).all() and cn.nodes.grad.abs().max() > 0
    off10 = 2 * net.hashgrid.encoding.level_table()[10][3]
    assert not gt[off10:].any() and gt[:off10].any()        # at step 3250 levels 10 and 11 are still masked out


def test_rejections():
    from riggs_amd import _lib as L
    from riggs_amd.control_nodes import ControlNodeWarp
    from riggs_amd.hash_network import HashDeformNetwork, HashGridEncoding
    with pytest.raises(L.RiggsHipError, match="n_features_per_level"):
        HashGridEncoding(3, {"n_features_per_level": 4})
    with pytest.raises(L.RiggsHipError, match="n_input_dims"):
        HashGridEncoding(2)
    with pytest.raises(NotImplementedError, match="tcnn_mlp"):
        HashDeformNetwork(tcnn_mlp=True)
    with pytest.raises(NotImplementedError, match="HashDeformNetwork"):
        ControlNodeWarp(use_hash=True)
    with pytest.raises(NotImplementedError, match="bbox"):
        ControlNodeWarp(use_hash=True, network=torch.nn.Linear(3, 3))
    enc = HashGridEncoding(3, CONFIGS["L5-base3"])
    with pytest.raises(L.RiggsHipError, match="CUDA"):
        enc(torch.rand(4, 3))
    with pytest.raises(L.RiggsHipError, match="detached"):
        enc(torch.rand(4, 3, device="cuda", requires_grad=True))
    with pytest.raises(L.RiggsHipError, match=r"\(R, 3\)"):
        enc(torch.rand(4, 4, device="cuda"))
    with pytest.raises(L.RiggsHipError, match="float32"):
        enc(torch.rand(4, 3, device="cuda").double())
    with pytest.raises(L.RiggsHipError, match="mask"):
        enc(torch.rand(4, 3, device="cuda"), torch.ones(9, device="cuda"))
    net = HashDeformNetwork(hidden_dim=64)
    with pytest.raises(L.RiggsHipError, match="CUDA"):
        net(torch.rand(4, 3), torch.rand(4, 1))
    with pytest.raises(L.RiggsHipError, match="detached"):
        net(torch.rand(4, 3, device="cuda", requires_grad=True), torch.rand(4, 1, device="cuda"))
    assert enc(torch.rand(0, 3, device="cuda")).shape == (0, 10)
