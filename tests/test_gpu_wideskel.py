"""-m gpu: skeletons of 65..256 joints — the workgroup-wide chain, the wide skinning kernels and the layered PoseMLP heads —
against golden vectors captured from the reference (tests/golden/make_wideskel_golden.py) and the CPU oracle."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import deform_ref as O  # noqa: E402
from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import synth  # noqa: E402
from riggs_amd.skeleton import SkeletonWarp, _DeformByPose, fk_forward  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests.test_gpu_deform import test_deform_matches_oracle_large as _oracle_large  # noqa: E402
from tests.test_gpu_deform import test_deform_matches_reference_golden as _golden  # noqa: E402
from tests.test_gpu_loss import test_skeleton_projection_loss_against_oracle as _skelproj  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WIDE = sorted(p for p in glob.glob(os.path.join(GOLD, "wideskel_*.npz")) if "posemlp" not in p)


def close(a, b, what, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.abs(a - b).max())
    assert err <= rel * max(1.0, float(np.abs(b).max())), "%s: max abs err %.3g" % (what, err)


@pytest.mark.parametrize("path", WIDE, ids=[os.path.basename(p)[:-4] for p in WIDE])
def test_wide_deform_matches_reference_golden(path):
    _golden(path)


def skeleton(J, chain, seed):
    g = torch.Generator().manual_seed(seed)
    if chain:
        parents = torch.arange(-1, J - 1)
        joints = torch.stack([torch.zeros(J), torch.linspace(-0.8, 0.8, J), torch.zeros(J)], -1) + 0.01 * torch.randn(J, 3, generator=g)
    else:
        parents = torch.full((J,), -1, dtype=torch.long)
        joints = torch.zeros(J, 3)
        for i in range(1, J):
            parents[i] = int(torch.randint(0, i, (1,), generator=g))
            joints[i] = joints[parents[i]] + 0.25 * torch.randn(3, generator=g)
    q = torch.tensor([1.0, 0, 0, 0]) + (0.02 if chain else 0.3) * torch.randn(J, 4, generator=g)
    return joints, parents, q, 0.02 * torch.randn(3, generator=g), g


@pytest.mark.parametrize("J", [65, 100, 256])
@pytest.mark.parametrize("chain", [False, True])
def test_fk_forward_backward_against_float64_oracle(J, chain):
    joints, parents, q, gt, g = skeleton(J, chain, 40 + J)
    dG, gn = torch.randn(J, 12, generator=g), torch.randn(J, 3, generator=g)
    # oracle in float64
    qd = q.double().requires_grad_(True)
    gtd = gt.double().requires_grad_(True)
    posed, G = O.fk_chain(O.quaternion_to_matrix(qd), joints.double(), parents)
    G12 = G[:, :3, :4].reshape(J, 12)
    d_nodes = posed + gtd
    ((G12 * dG.double()).sum() + (d_nodes * gn.double()).sum()).backward()
    # HIP
    p32 = parents.to(torch.int32).cuda()
    jc, qc, gtc = joints.cuda(), q.cuda(), gt.cuda()
    tr, nrot, dn = fk_forward(qc, jc, p32, gtc)
    dq = torch.empty(J, 4, device="cuda")
    dgt = torch.zeros(3, device="cuda")
    dGc, gnc = dG.cuda(), gn.cuda()  # (held: a temporary's memory could be handed to the next one before the launch runs)
    L.check(L.lib().riggs_fk_backward(J, qc.data_ptr(), jc.data_ptr(), p32.data_ptr(), dGc.data_ptr(), gnc.data_ptr(),
                                      dq.data_ptr(), dgt.data_ptr(), L.stream_ptr()), "riggs_fk_backward")
    torch.cuda.synchronize()
    rel = 1e-4 if not chain else 2e-4
    close(tr.cpu(), G12.detach(), "transforms", rel)
    close(dn.cpu(), d_nodes.detach(), "d_nodes", rel)
    close(nrot.cpu(), O.matrix_to_quaternion(G[:, :3, :3].detach().float()), "node_rot", 1e-4)
    close(dq.cpu(), qd.grad, "dL/dlocal_rot", 2e-4 if not chain else 1e-3)
    close(dgt.cpu(), gtd.grad, "dL/dglobal_trans", 1e-5)


def test_deform_large_tree_200_joints_matches_oracle():
    _oracle_large(300_000, 200, False, 1239)


def test_deform_with_weight_mod_at_200_joints_matches_oracle():
    N, J, seed = 300_000, 200, 1240
    sc = synth.make_scene(N, J, seed)
    g = torch.Generator().manual_seed(seed)
    gx, gr, gn = torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g), torch.randn(J, 3, generator=g)
    wm = torch.sigmoid(torch.randn(N, J - 1, generator=g))
    mask = torch.rand(N, 1, generator=g)
    q = sc["local_rotation"].clone().requires_grad_(True)
    gt = sc["global_trans"].clone().requires_grad_(True)
    rho = sc["node_radius"].clone().requires_grad_(True)
    wo = wm.clone().requires_grad_(True)
    mo = mask.clone().requires_grad_(True)
    o = O.deform_by_pose(sc["xyz"], sc["joints"], sc["parents"], rho, q, gt, mo, -1, weight_offsets=wo)
    ((o["d_xyz"] * gx).sum() + (o["d_rotation"] * gr).sum() + (o["d_nodes"] * gn).sum()).backward()
    qh = sc["local_rotation"].cuda().requires_grad_(True)
    gth = sc["global_trans"].cuda().requires_grad_(True)
    rhoh = sc["node_radius"].cuda().requires_grad_(True)
    wh = wm.cuda().requires_grad_(True)
    mh = mask.cuda().requires_grad_(True)
    p32 = sc["parents"].to(torch.int32).cuda()
    d_xyz, d_rot, d_nodes, _, _ = _DeformByPose.apply(qh, gth, rhoh, mh, sc["xyz"].cuda(), sc["joints"].cuda(), p32, -1, wh)
    ((d_xyz * gx.cuda()).sum() + (d_rot * gr.cuda()).sum() + (d_nodes * gn.cuda()).sum()).backward()
    U.assert_close(d_xyz.detach().cpu().numpy(), o["d_xyz"].detach().numpy(), "d_xyz")
    U.assert_close(d_rot.detach().cpu().numpy(), o["d_rotation"].detach().numpy(), "d_rotation")
    U.assert_close(d_nodes.detach().cpu().numpy(), o["d_nodes"].detach().numpy(), "d_nodes", 1e-5)
    U.assert_close(qh.grad.cpu().numpy(), q.grad.numpy(), "dL/dlocal_rotation", 2e-4)
    U.assert_close(gth.grad.cpu().numpy(), gt.grad.numpy(), "dL/dglobal_trans", 2e-4)
    U.assert_close(rhoh.grad.cpu().numpy(), rho.grad.numpy(), "dL/d_node_radius", 2e-4)
    U.assert_close(wh.grad.cpu().numpy(), wo.grad.numpy(), "dL/dweight_mod", 2e-4)
    U.assert_close(mh.grad.cpu().numpy(), mo.grad.numpy(), "dL/dmotion_mask", 2e-4)


@pytest.mark.parametrize("J", [128, 200])
def test_layered_pose_mlp_matches_torch(J):
    from riggs_amd.skeleton import PoseMLP
    torch.manual_seed(6)
    net = PoseMLP(1, J * 4, depth=8, hidden_dimensions=256, multires=8)
    t = torch.tensor([0.37])
    ref = net(t)
    gr, gtr = torch.randn(J * 4), torch.randn(3)
    (ref["rotation"] * gr).sum().add((ref["translation"] * gtr).sum()).backward()
    net_g = copy.deepcopy(net).cuda()
    for p in net_g.parameters():
        p.grad = None
    out = net_g(t.cuda())
    (out["rotation"] * gr.cuda()).sum().add((out["translation"] * gtr.cuda()).sum()).backward()
    U.assert_close(out["rotation"].detach().cpu().numpy(), ref["rotation"].detach().numpy(), "rotation", 1e-5)
    U.assert_close(out["translation"].detach().cpu().numpy(), ref["translation"].detach().numpy(), "translation", 1e-5)
    for (n, p), q in zip(net.named_parameters(), net_g.parameters()):
        U.assert_close(q.grad.cpu().numpy(), p.grad.numpy(), "grad " + n, 1e-4)


def test_pose_mlp_matches_reference_fixture_at_128_joints():
    from riggs_amd.skeleton import PoseMLP
    g = np.load(os.path.join(GOLD, "wideskel_posemlp_j128.npz"))
    net = PoseMLP(1, 128 * 4, depth=8, hidden_dimensions=32, multires=8)
    net.load_state_dict({k.replace("__", "."): torch.from_numpy(g[k]) for k in g.files if "__" in k})
    out = net.cuda()(torch.from_numpy(g["t"]).cuda())
    U.assert_close(out["rotation"].detach().cpu().numpy(), g["rotation"], "rotation vs reference", 1e-5)
    U.assert_close(out["translation"].detach().cpu().numpy(), g["translation"], "translation vs reference", 1e-5)


@pytest.mark.parametrize("J,heads", [(128, False), (200, False), (128, True)])
def test_forward_as_one_node_matches_pose_net_plus_deform_by_pose(J, heads):
    """SkeletonWarp.forward (PoseMLP, chain + skinning, and backward riggs_pose_mlp_backward_fk as one autograd node: the
    torch-extension pose_deform where it is built) against get_pose_info + deform_by_pose."""
    sc = synth.make_scene(3000, J, 7)
    torch.manual_seed(3)
    sw = SkeletonWarp(joints=sc["joints"], parent_indices=sc["parents"], K=-1, hyper_dim=8, use_skinning_weight_mlp=heads,
                      use_template_offsets=heads).cuda()
    sw._node_radius.data = sc["node_radius"].cuda()
    x = sc["xyz"].cuda()
    mask = torch.rand(x.shape[0], 1, device="cuda")
    t = torch.tensor(0.41, device="cuda")
    g = torch.Generator().manual_seed(1)
    w_xyz, w_rot, w_nodes = (torch.randn(s, generator=g).cuda() for s in ((x.shape[0], 3), (x.shape[0], 4), (J, 3)))

    def run(fused):
        for p in sw.parameters():
            p.grad = None
        dv = sw(x, t, mask) if fused else sw.deform_by_pose(x, sw.get_pose_info(sw.expand_time(t)), mask)
        loss = (dv["d_xyz"] * w_xyz).sum() + (dv["d_rotation"] * w_rot).sum() + (dv["d_nodes"] * w_nodes).sum() \
            + 0.1 * (dv["local_rotation"] ** 2).sum() + 0.3 * dv["global_trans"].sum()
        loss.backward()
        return ({k: dv[k].detach().clone() for k in ("d_xyz", "d_rotation", "d_nodes", "local_rotation", "global_trans")},
                {n: p.grad.detach().clone() for n, p in sw.named_parameters() if p.grad is not None})

    o1, g1 = run(True)
    o0, g0 = run(False)
    for k in o0:
        assert torch.isfinite(o1[k]).all(), k
        assert float((o1[k] - o0[k]).abs().max()) <= 1e-6 * max(1.0, float(o0[k].abs().max())), k
    assert set(g0) == set(g1) and len(g0) >= 20
    for n in g0:
        assert float((g1[n] - g0[n]).abs().max()) <= 2e-5 * max(1e-9, float(g0[n].abs().max())), n


def test_torch_extension_pose_deform_at_128_joints():
    from riggs_amd import _torch_ext
    assert _torch_ext.available()
    test_forward_as_one_node_matches_pose_net_plus_deform_by_pose(128, True)


def test_skeleton_projection_loss_at_200_joints():
    _skelproj(200, 5000, 512, 7)


def test_graphed_train_step_matches_eager_iterations_at_128_joints():
    from types import SimpleNamespace

    import bench
    from riggs_amd.graph import GraphedTrainStep
    from riggs_amd.loss import l1_loss, ssim
    from riggs_amd.optim import FusedAdam
    from riggs_amd.rasterizer import RasterArena
    from riggs_amd.render import render
    old = dict(bench.WORKLOAD)
    bench.WORKLOAD.update(N=5000, J=128, H=80, W=96)
    args = SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                           position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.001, rotation_lr=0.001)
    try:
        sc, cam, gm, sw = bench.build_workload(0, "cuda:0")
        assert sw.nodes.shape[0] == 128
        gm2, sw2 = copy.deepcopy(gm), copy.deepcopy(sw)
        gt = torch.rand(3, 80, 96, generator=torch.Generator().manual_seed(2)).cuda()
        bg = torch.zeros(3, device="cuda")
        gm.training_setup(args, capturable=True)
        sk_opt = FusedAdam([{"params": g["params"], "lr": 5e-4, "name": g["name"]} for g in sw.trainable_parameters()],
                           lr=0.0, eps=1e-15, capturable=True)
        gts = GraphedTrainStep(gm, sw, cam, bg, gt, [gm.optimizer, sk_opt], lambda_dssim=0.2)
        gts.capture(warmup=1)
        losses = []
        for it in range(2, 5):
            gm.update_learning_rate(1000 * it)
            out = gts.run()
            losses.append(out["loss"].item())
        gts.check()
        gm2.training_setup(args)
        opt_g = torch.optim.Adam([{"params": g["params"], "lr": float(g["lr"]), "name": g["name"]} for g in gm2.optimizer.param_groups],
                                 lr=0.0, eps=1e-15)
        opt_s = torch.optim.Adam([{"params": g["params"], "lr": 5e-4} for g in sw2.trainable_parameters()], lr=0.0, eps=1e-15)
        ref_losses = []
        for it in range(1, 5):
            if it >= 2:
                for grp in opt_g.param_groups:
                    if grp["name"] == "xyz":
                        grp["lr"] = gm2.xyz_scheduler_args(1000 * it)
            opt_g.zero_grad(set_to_none=True), opt_s.zero_grad(set_to_none=True)
            dv = sw2(gm2.get_xyz.detach(), sw2.expand_time(cam.fid), motion_mask=gm2.motion_mask)
            pkg = render(cam, gm2, bench.Pipe, bg, dv["d_xyz"], dv["d_rotation"], dv["d_scaling"], arena=RasterArena())
            loss = 0.8 * l1_loss(pkg["render"], gt) + 0.2 * (1.0 - ssim(pkg["render"], gt))
            loss.backward()
            opt_g.step(), opt_s.step()
            if it >= 2:
                ref_losses.append(loss.item())
        np.testing.assert_allclose(losses, ref_losses, rtol=2e-4)
        for a, b in zip(gm.parameters(), gm2.parameters()):
            a, b = a.detach(), b.detach()
            bad = (a - b).abs() > 2e-3 * b.abs() + 2e-4 * float(b.abs().max())
            assert float(bad.float().mean()) <= 1e-3, float(bad.float().mean())
    finally:
        bench.WORKLOAD.clear()
        bench.WORKLOAD.update(old)
