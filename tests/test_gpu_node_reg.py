"""Stage-1 node regularisers on the GPU (csrc/node_reg.hip through riggs_amd.node_reg and ControlNodeWarp): the float64
restatement (tests/node_reg_ref.py) over node counts, time samples and hyper dimensions with ties and dropped edges; the
reg_loss schedule; no host synchronisation; bitwise repeatability; rejections; a short stage-1 schedule with densification
and a state_dict round trip."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from tests import node_reg_ref as R

pytestmark = pytest.mark.gpu


def _close(got, ref, rel, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((got - ref).abs().max())
    assert err <= rel * scale, "%s: max err %.3g vs scale %.3g" % (what, err, scale)


def _nodes(M, hyper, seed, dup=True):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(M, 3, generator=g) * (0.05 * max(M, 8) ** (1 / 3))
    if dup and M > 4:  # duplicated nodes: exact ties in every distance to them
        k = max(1, M // 10)
        xyz[M - k:] = xyz[:k]
    h = 1e-2 + 0.02 * torch.randn(M, hyper, generator=g)
    return torch.cat([xyz, h], -1), g


@pytest.mark.parametrize("M", [1, 11, 512, 1024, 8192])
@pytest.mark.parametrize("T", [2, 3, 8])
@pytest.mark.parametrize("hyper", [0, 8])
def test_regularisers_match_float64_restatement(M, T, hyper):
    from riggs_amd import node_reg as NR
    nodes, g = _nodes(M, hyper, 1000 * M + 10 * T + hyper)
    nodes = nodes.cuda()
    seq0 = nodes[:, :3]
    disp = 0.02 * torch.randn(T, M, 3, generator=g).cuda()
    disp[:, :: 7] = 0.0  # nodes that do not move: rows whose edges keep coordinates unchanged
    seq = (seq0[None] + disp).contiguous()
    # connectivity: index lists exact (dropped edges beyond the radius included)
    idx, dist = NR.connectivity_padded(seq[0], K=10)
    ridx, rdist = R.knn_ref(seq[0], 11, drop_first=True, least_edge_num=3, radius=0.1)
    assert torch.equal(idx.long().cpu(), ridx.cpu())
    assert torch.equal(dist.cpu(), rdist.cpu())
    if M >= 64:
        assert (idx < 0).any() and (idx >= 0).any()
    # ARAP: value and gradient with the kernel's own sample rows
    rows = NR.arap_sample_rows(M, device="cuda")
    s = seq.clone().requires_grad_(True)
    e = NR.arap_error_padded(s, idx, rows=rows)
    go = torch.tensor(0.7, device="cuda")
    (e * go).backward()
    s64 = seq.double().requires_grad_(True)
    e64 = R.arap_ref(s64, ridx.cuda(), rows.long())
    (e64 * 0.7).backward()
    _close(e, e64, 1e-5, "arap value")
    _close(s.grad, s64.grad, 1e-4, "arap grad")
    # elastic over the (xyz, hyper) graph with differentiable weights
    K = 2 if T != 8 else 5
    kidx, _ = NR.node_knn(nodes, K + 1)
    rk, _ = R.knn_ref(nodes, K + 1)
    assert torch.equal(kidx.long().cpu(), rk.cpu())
    radius = (math.log(0.15) + 0.3 * torch.randn(M, generator=g)).cuda()
    wl = (0.5 * torch.randn(M, 1, generator=g)).cuda()
    nt = seq.permute(1, 0, 2).contiguous()
    p = [nodes.clone().requires_grad_(True), radius.clone().requires_grad_(True), wl.clone().requires_grad_(True),
         nt.clone().requires_grad_(True)]
    w = NR.node_graph_weight(p[0], p[1], p[2], hyper, kidx)
    le = NR.elastic_energy(p[3], kidx[:, 1:].contiguous(), w[:, 1:])
    le.backward()
    q = [t.double().requires_grad_(True) for t in (nodes, radius, wl, nt)]
    w64 = R.graph_weight_ref(q[0], q[1], q[2], hyper, rk.cuda())
    le64 = R.elastic_ref(q[3], rk.cuda()[:, 1:], w64[:, 1:])
    le64.backward()
    _close(le, le64, 1e-5, "elastic value")
    for a, b, n in zip(p, q, ("nodes", "radius", "weight", "nodes_t")):
        _close(a.grad if a.grad is not None else torch.zeros_like(a), b.grad if b.grad is not None else torch.zeros_like(b), 1e-4,
               "elastic grad " + n)
    # acceleration (the still nodes: a norm of exactly zero)
    a3 = seq[:3].permute(1, 0, 2).contiguous() if T >= 3 else torch.cat([seq, seq[:1]]).permute(1, 0, 2).contiguous()
    pa = a3.clone().requires_grad_(True)
    la = NR.acc_energy(pa)
    la.backward()
    pa64 = a3.double().requires_grad_(True)
    la64 = R.acc_ref(pa64)
    la64.backward()
    _close(la, la64, 1e-5, "acc value")
    _close(pa.grad, pa64.grad, 1e-4, "acc grad")


def test_arap_samples_512_rows_with_replacement():
    from riggs_amd import node_reg as NR
    torch.manual_seed(3)
    r = torch.stack([NR.arap_sample_rows(600, device="cuda") for _ in range(200)]).long().cpu()
    assert r.shape == (200, 512) and int(r.min()) >= 0 and int(r.max()) < 600
    counts = torch.bincount(r.reshape(-1), minlength=600).double()
    assert float(counts.std() / counts.mean()) < 0.1  # uniform: expected 0.0588
    assert any(len(set(x.tolist())) < 512 for x in r)  # with replacement
    assert torch.equal(NR.arap_sample_rows(512, device="cuda").cpu(), torch.arange(512, dtype=torch.int32))


def test_zero_covariance_gives_identity_and_zero_energy():
    from riggs_amd import node_reg as NR
    nodes, _ = _nodes(64, 0, 5, dup=False)
    seq = nodes[:, :3].cuda()[None].expand(3, 64, 3).contiguous()
    idx, _ = NR.connectivity_padded(seq[0], K=10)
    e = NR.arap_error_padded(seq, idx)
    assert float(e) == 0.0


class _NodeNet(nn.Module):
    """A closed-form node network with parameters: d_xyz = A sin(2 pi f t + phase(x)) + B x t."""

    def __init__(self):
        super().__init__()
        self.A = nn.Parameter(torch.tensor([0.05, -0.03, 0.02]))
        self.B = nn.Parameter(0.1 * torch.eye(3))
        self.f = nn.Parameter(torch.tensor(1.3))
        self.register_buffer("phase", torch.tensor([1.0, 2.0, -1.0]))

    def forward(self, x, t, **kwargs):
        ph = x @ self.phase
        d = self.A * torch.sin(2 * math.pi * self.f * t + ph[:, None]) + t * (x @ self.B)
        z4 = torch.zeros(x.shape[0], 4, device=x.device)
        return {"d_xyz": d, "d_rotation": z4 + 0.01 * d[:, :1], "d_scaling": 0.1 * d, "local_rotation": z4.clone(), "hidden": None,
                "d_opacity": None, "d_color": None}


def _warp(M=300, hyper=8, **kw):
    from riggs_amd.control_nodes import ControlNodeWarp
    cn = ControlNodeWarp(node_num=M, K=3, hyper_dim=hyper, network=_NodeNet(), **kw).cuda()
    nodes, g = _nodes(M, hyper, 77)
    cn.nodes.data = nodes.cuda()
    cn._node_radius.data = (math.log(0.15) + 0.3 * torch.randn(M, generator=g)).cuda()
    cn._node_weight.data = (0.5 * torch.randn(M, 1, generator=g)).cuda()
    return cn


def test_reg_loss_schedule():
    cn = _warp(with_arap_loss=True)
    x = torch.rand(500, 3, device="cuda") * 0.3
    feat = 0.02 * torch.randn(500, 9, device="cuda")
    want = {0: 1e-4, 4999: 1e-4, 10000: 1e-5, 19999: 1e-5, 20000: 0.0}
    for it, lam in want.items():
        torch.manual_seed(it)
        cn(x, torch.tensor(0.4, device="cuda"), feat, 1.0, iteration=it)
        if lam == 0.0:
            assert isinstance(cn.reg_loss, float) and cn.reg_loss == 0.0
        else:
            torch.manual_seed(it)
            t = torch.tensor(0.4, device="cuda")
            _ = cn.node_deform(t=cn.expand_time(t))  # (no random numbers drawn)
            torch.manual_seed(it)
            ref = cn.arap_loss() * lam
            assert torch.is_tensor(cn.reg_loss) and cn.reg_loss.requires_grad
            assert abs(float(cn.reg_loss.detach()) - float(ref.detach())) <= 1e-6 * abs(float(ref)) + 1e-30
    cn(x, torch.tensor(0.4, device="cuda"), feat, 1.0, iteration=0, is_training=False)
    assert cn.reg_loss == 0.0
    cn.eval()
    cn(x, torch.tensor(0.4, device="cuda"), feat, 1.0, iteration=0)
    assert cn.reg_loss == 0.0
    off = _warp()  # with_arap_loss off (the default): unchanged behaviour
    off(x, torch.tensor(0.4, device="cuda"), feat, 1.0, iteration=0)
    assert off.reg_loss == 0.0


def _losses(cn, seed, t):
    torch.manual_seed(seed)
    for p in cn.parameters():
        p.grad = None
    loss = cn.arap_loss() + 1e-3 * cn.elastic_loss(t=t, delta_t=0.01) + 1e-5 * cn.acc_loss(t=t, delta_t=0.03)
    loss.backward()
    return loss.detach().clone(), [p.grad.clone() for p in cn.parameters() if p.grad is not None]


@pytest.mark.parametrize("M", [300, 2000])
def test_no_host_sync_and_bitwise_repeatable(M):
    cn = _warp(M=M)
    t = torch.tensor(0.3, device="cuda")  # (a host-to-device copy: before the checked region)
    _losses(cn, 1, t)  # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # positive control: the mode is honoured by this build
            torch.zeros(1, device="cuda").item()
        a = _losses(cn, 11, t)
        b = _losses(cn, 11, t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) >= 5
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    assert torch.isfinite(a[0]) and all(torch.isfinite(g).all() for g in a[1])


def test_rejections():
    from riggs_amd import _lib as L
    from riggs_amd import node_reg as NR
    from riggs_amd.control_nodes import ControlNodeWarp
    with pytest.raises(NotImplementedError):
        ControlNodeWarp(use_hash=True)
    with pytest.raises(L.RiggsHipError):
        NR.node_knn(torch.rand(10, 3), 4)
    with pytest.raises(L.RiggsHipError):
        NR.acc_energy(torch.rand(10, 3, 3))
    x = torch.rand(20, 4, 3, device="cuda")
    with pytest.raises(L.RiggsHipError):  # K > 15
        NR.elastic_energy(x, torch.zeros(20, 16, dtype=torch.int32, device="cuda"), torch.ones(20, 16, device="cuda"))
    with pytest.raises(L.RiggsHipError):  # K + 1 > 16 neighbour columns
        NR.node_knn(torch.rand(40, 3, device="cuda"), 17)
    with pytest.raises(L.RiggsHipError):  # M > 8192
        NR.acc_energy(torch.rand(8193, 3, 3, device="cuda"))
    with pytest.raises(L.RiggsHipError):  # T > 16
        NR.arap_error_padded(torch.rand(17, 20, 3, device="cuda"), torch.zeros(20, 10, dtype=torch.int32, device="cuda"))
    with pytest.raises(NotImplementedError):
        NR.cal_connectivity_from_points(torch.rand(20, 3, device="cuda"), mode="floyd")


def test_connectivity_reference_signature():
    from riggs_amd import node_reg as NR
    nodes, _ = _nodes(64, 0, 9)
    p = nodes[:, :3].cuda()
    ii, jj, nn_, w = NR.cal_connectivity_from_points(p, K=10)
    ridx, rdist = R.knn_ref(p, 11, drop_first=True, least_edge_num=3, radius=0.1)
    keep = ridx.reshape(-1) != -1
    assert torch.equal(jj.cpu(), ridx.reshape(-1)[keep].cpu())
    assert torch.equal(ii.cpu(), torch.arange(64)[:, None].expand(64, 10).reshape(-1)[keep.cpu()])
    assert torch.equal(nn_.cpu(), torch.arange(10)[None].expand(64, 10).reshape(-1)[keep.cpu()])
    assert bool((~keep).any())
    ww = torch.exp(-rdist / rdist.mean())
    ww = ww / ww.sum(-1, keepdim=True)
    assert torch.equal(torch.isnan(w).cpu(), torch.isnan(ww).cpu()) and bool(torch.isnan(w).any())
    e = NR.cal_arap_error(torch.stack([p, p + 0.01 * torch.randn_like(p)]), ii, jj, nn_)
    assert torch.isfinite(e) and float(e) > 0


class _Opt:
    position_lr_init = position_lr_final = 1e-4
    position_lr_delay_mult = 0.01
    position_lr_max_steps = 1000
    feature_lr = opacity_lr = scaling_lr = rotation_lr = 1e-3
    percent_dense = 0.01


def test_short_stage1_schedule():
    """train_gui.py's node phase call by call with shrunk thresholds: init from a point cloud, node-rendering steps with the
    node regularisers after the warm-up, Gaussian steps through forward(iteration=) with reg_loss, a forced densify."""
    from riggs_amd.control_nodes import ControlNodeWarp
    torch.manual_seed(0)
    pcl = torch.rand(2000, 3, device="cuda") * 0.4
    cn = ControlNodeWarp(node_num=128, K=3, hyper_dim=8, network=_NodeNet(), with_arap_loss=True, is_blender=True).cuda()
    assert cn.name == "node" and not bool(cn.inited)
    idx = cn.init(_Opt(), pcl, hyper_pcl=None, force_init=True, as_gs_force_with_motion_mask=False, force_gs_keep_all=False)
    assert bool(cn.inited) and idx.shape == (128,) and cn.nodes.shape == (128, 11)
    assert cn.as_gaussians.get_xyz.shape == (128, 3)
    opt = torch.optim.Adam(cn.trainable_parameters(), lr=1e-3)
    warm_up, force_step = 3, 8
    feat = (0.02 * torch.randn(2000, 9, device="cuda")).requires_grad_(True)
    for it in range(12):
        cn.update(it)
        fid = torch.rand((), device="cuda")
        if it < 6:  # node rendering phase: the nodes' own Gaussians (train_gui.py:1224-1311)
            out = cn.query_network(x=cn.nodes[:, :3].detach(), t=fid.expand(cn.node_num, 1))
            loss = (cn.as_gaussians.get_xyz + out["d_xyz"]).square().mean()
            if it > warm_up:
                loss = loss + 1e-3 * cn.elastic_loss(t=fid, delta_t=0.01) + 1e-5 * cn.acc_loss(t=fid, delta_t=0.03)
                loss = loss + 1e-2 * cn.arap_loss()
        else:  # Gaussian phase (train_gui.py:1030-1216)
            d = cn(pcl, fid, feat, 1.0, iteration=it)
            loss = d["d_xyz"].square().mean() + d["d_scaling"].square().mean() + cn.reg_loss
        opt.zero_grad()
        loss.backward()
        assert torch.isfinite(loss)
        opt.step()
        if it == force_step:
            grad = torch.rand(2000, 3, device="cuda") * 1e-3
            grad[:50] = 1.0  # some Gaussians with large gradients: their nodes split
            n0 = cn.node_num
            cn.densify(max_grad=1e-2, optimizer=opt, x=pcl, x_grad=grad, feature=feat.detach(), force_dp=True)
            assert cn.node_num != n0
            grp = [g for g in opt.param_groups if g["name"] == "nodes"][0]
            for name, p in zip(cn.param_names, grp["params"]):
                assert p is getattr(cn, name) and p.shape[0] == cn.node_num
                st = opt.state[p]
                assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
            assert cn.as_gaussians.get_xyz.shape[0] == cn.node_num
            assert cn.nodes_color_visualization.shape[0] == cn.node_num
            assert cn.as_gaussians._xyz.data_ptr() == cn.nodes.data_ptr()  # the _xyz = nodes[..., :3] alias
    sd = cn.state_dict()
    assert any(k.startswith("gs_") for k in sd) and "inited" in sd
    other = ControlNodeWarp(node_num=16, K=3, hyper_dim=8, network=_NodeNet(), with_arap_loss=True).cuda()
    other.load_state_dict({k: v.clone() for k, v in sd.items()})
    for name in cn.param_names:
        assert torch.equal(getattr(other, name).data, getattr(cn, name).data)
    assert bool(other.inited)
    x = torch.rand(100, 3, device="cuda")
    a = cn(x, torch.tensor(0.5, device="cuda"), feat[:100].detach(), 1.0, is_training=False)
    b = other(x, torch.tensor(0.5, device="cuda"), feat[:100].detach(), 1.0, is_training=False)
    assert torch.equal(a["d_xyz"], b["d_xyz"])


def test_module_matches_reference_arap_fixture():
    import os
    from riggs_amd import node_reg as NR
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "stage1_arap_m64_t3.npz"))
    seq = torch.from_numpy(z["seq"]).cuda()
    ii, jj, nn_, w = NR.cal_connectivity_from_points(seq[0], K=10)
    assert torch.equal(ii.cpu(), torch.from_numpy(z["ii"])) and torch.equal(jj.cpu(), torch.from_numpy(z["jj"]))
    assert torch.equal(nn_.cpu(), torch.from_numpy(z["nn"]))
    wg = w.cpu().numpy()
    assert np.array_equal(np.isnan(wg), np.isnan(z["weight"]))
    ok = ~np.isnan(wg)
    if ok.any():
        assert np.abs(wg[ok] - z["weight"][ok]).max() <= 1e-6
    s = seq.clone().requires_grad_(True)
    e = NR.cal_arap_error(s, ii, jj, nn_)
    e.backward()
    assert abs(float(e) - float(z["arap"])) <= 1e-5 * abs(float(z["arap"]))
    g = z["grad_seq"]
    assert np.abs(s.grad.cpu().numpy() - g).max() <= 1e-4 * np.abs(g).max()


def test_out_of_range_indices_count_as_dropped_edges():
    from riggs_amd import node_reg as NR
    nodes, _ = _nodes(40, 0, 12, dup=False)
    seq = (nodes[:, :3][None] + 0.01 * torch.randn(3, 40, 3)).cuda()
    idx, _ = NR.connectivity_padded(seq[0], K=10)
    bad = idx.clone()
    bad[3, 4], bad[7, 0] = 40, 1 << 30  # beyond M: dropped, as -1 would be
    ref = idx.clone()
    ref[3, 4], ref[7, 0] = -1, -1
    rows = torch.tensor([0, 5, 40, 39, -2], dtype=torch.int32, device="cuda")
    ref_rows = torch.tensor([0, 5, 39], dtype=torch.int32, device="cuda")
    assert float(NR.arap_error_padded(seq, bad, rows=rows)) == float(NR.arap_error_padded(seq, ref, rows=ref_rows))
    nt = seq.permute(1, 0, 2).contiguous()
    w = torch.rand(40, 10, device="cuda")
    assert float(NR.elastic_energy(nt, bad, w)) == float(NR.elastic_energy(nt, ref, w))
    ii, jj, nn_, _ = NR.cal_connectivity_from_points(seq[0], K=10)
    with pytest.raises(Exception):
        NR.cal_arap_error(seq, ii + 1000, jj, nn_)


def _golden(name):
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))


def test_module_matches_reference_arap_fixture_with_recorded_sample():
    """(b) M = 600 > 512: the reference's np.random.choice rows, replayed."""
    from riggs_amd import node_reg as NR
    z = _golden("stage1_arap_m600_t3")
    seq = torch.from_numpy(z["seq"]).cuda()
    ii, jj, nn_, _ = NR.cal_connectivity_from_points(seq[0], K=10)
    assert torch.equal(ii.cpu(), torch.from_numpy(z["ii"])) and torch.equal(jj.cpu(), torch.from_numpy(z["jj"]))
    assert torch.equal(nn_.cpu(), torch.from_numpy(z["nn"]))
    idx, _ = NR.connectivity_padded(seq[0], K=10)
    s = seq.clone().requires_grad_(True)
    e = NR.arap_error_padded(s, idx, rows=torch.from_numpy(z["rows"]).cuda())
    e.backward()
    assert z["rows"].shape == (512,)
    _close(e, torch.tensor(float(z["arap"])), 1e-5, "arap value")
    _close(s.grad, torch.from_numpy(z["grad_seq"]), 1e-4, "arap grad")


def _replay_warp(z, replay):
    from riggs_amd.control_nodes import ControlNodeWarp
    net = R.ClosedFormNodeNet()
    for k, p in net.named_parameters():
        p.data = torch.from_numpy(z["net_" + k])
    M = z["nodes"].shape[0]
    cn = ControlNodeWarp(node_num=M, K=3, hyper_dim=8, with_node_weight=True, network=R.TimeReplay(net, replay)).cuda()
    cn.nodes.data = torch.from_numpy(z["nodes"]).cuda()
    cn._node_radius.data = torch.from_numpy(z["_node_radius"]).cuda()
    cn._node_weight.data = torch.from_numpy(z["_node_weight"]).cuda()
    return cn


@pytest.mark.parametrize("loss", ["arap", "elastic", "acc"])
def test_module_losses_match_reference_fixture(loss):
    """(c) the reference ControlNodeWarp's losses at the time samples it drew: value and every parameter gradient."""
    z = _golden("stage1_losses_m300")
    cn = _replay_warp(z, [torch.from_numpy(t) for t in z[loss + "_t"]])
    kw = {"arap": dict(delta_t=0.5, t_samp_num=3), "elastic": dict(t=torch.tensor(0.4, device="cuda"), delta_t=0.05),
          "acc": dict(t=torch.tensor(0.4, device="cuda"), delta_t=0.1)}[loss]
    v = getattr(cn, loss + "_loss")(**kw)
    v.backward()
    assert len(cn.network.seen) == z[loss + "_t"].shape[0]
    _close(v, torch.tensor(float(z[loss])), 1e-5, loss + " value")
    named = [(k, p) for k, p in cn.network.net.named_parameters()] + [("nodes", cn.nodes), ("_node_radius", cn._node_radius),
                                                                      ("_node_weight", cn._node_weight)]
    # scale: the tensor's largest gradient, at least 1 % of the loss's largest one (acc's gradient to B is zero in exact
    # arithmetic: the fp32 reference and the kernel both hold rounding noise there)
    gmax = max(float(np.abs(z[loss + "_grad_" + k]).max()) for k, _ in named)
    for k, p in named:
        ref = torch.from_numpy(z[loss + "_grad_" + k])
        got = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().cpu()
        err = float((got - ref.double()).abs().max())
        assert err <= 1e-4 * max(float(ref.abs().max()), 1e-2 * gmax), (loss, k, err)


def test_module_init_importance_densify_match_reference_fixture(monkeypatch):
    """(d) init from the recorded farthest-point start, cal_node_importance, one Adam step, densify(force_dp=True)."""
    import functools
    from riggs_amd import gaussian_model as GM
    from riggs_amd.control_nodes import ControlNodeWarp
    z = _golden("stage1_densify_m64")
    monkeypatch.setattr(GM, "farthest_point_sample", functools.partial(GM.farthest_point_sample, start=[int(z["fps_start"])]))
    cn = ControlNodeWarp(node_num=64, K=3, hyper_dim=8, with_node_weight=True, network=R.ClosedFormNodeNet(),
                         enable_densify_prune=True).cuda()
    x, pcl, feature, x_grad = (t.cuda() for t in R.densify_inputs(8))
    idx = cn.init(R.DensifyOpt(), pcl)
    assert torch.equal(idx.cpu(), torch.from_numpy(z["init_idx"]))
    opt = torch.optim.Adam(cn.trainable_parameters(), lr=1e-3, eps=1e-15)
    R.densify_step_loss(cn).backward()
    opt.step()
    imp, avg_x, cnt = cn.cal_node_importance(x=x, K=3, weights=x_grad.norm(dim=-1), feature=feature)
    _close(imp, torch.from_numpy(z["importance"]), 1e-5, "importance")
    _close(cnt, torch.from_numpy(z["edge_count"]), 1e-5, "edge count")
    ok = torch.from_numpy(~np.isnan(z["avg_x"]).any(-1))
    assert torch.equal(torch.isnan(avg_x).any(-1).cpu(), ~ok)
    _close(avg_x.cpu()[ok], torch.from_numpy(z["avg_x"])[ok], 1e-5, "avg x")
    cn.densify(max_grad=0.02, optimizer=opt, x=x, x_grad=x_grad.clone(), feature=feature, force_dp=True)
    assert cn.nodes.shape == z["nodes"].shape
    for k in ("nodes", "_node_radius", "_node_weight"):
        _close(getattr(cn, k), torch.from_numpy(z[k]), 1e-5, k)
    assert torch.equal(cn.nodes_color_visualization.cpu(), torch.from_numpy(z["color"]))
    grp = [g for g in opt.param_groups if g["name"] == "nodes"][0]
    for k, p in zip(cn.param_names, grp["params"]):
        assert p is getattr(cn, k)
        for m in ("exp_avg", "exp_avg_sq"):
            ref = torch.from_numpy(z[m + "_" + k])
            got = opt.state[p][m]
            assert got.shape == ref.shape, (m, k)
            _close(got, ref, 1e-5, m + " " + k)
            n_new = z["nodes"].shape[0] - 64 + int((z["edge_count"] == 0).sum())
            assert n_new > 0 and float(got[-n_new:].abs().max()) == 0.0  # the rows densify appended start with zero moments
    for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        ref = torch.from_numpy(z["gs" + k])
        got = getattr(cn.as_gaussians, k).detach()
        assert got.shape == ref.shape, k
        if ref.numel():
            _close(got, ref, 1e-5, "gs" + k)
