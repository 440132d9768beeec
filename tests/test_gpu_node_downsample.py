"""GPU: the stage-1 node sampling step (train_gui.py:1334-1370) on ``ControlNodeWarp`` — ``hyper_trajectories`` is the reference's
statement sequence over the library's own ``query_network``; ``downsample('samp_hyper')`` picks by the wide farthest-point sampler
and gathers the picked node Gaussians' parameters; ``with_dynamic_mask`` picks from the dynamic half only; ``'direct'`` keeps all
and shares the storage; too few masked points are refused.  700 node Gaussians, 64 nodes, the width-64 node network."""
import pytest
import torch

from tests import node_mlp_ref as NR
from tests.node_reg_ref import DensifyOpt as _Opt

pytestmark = pytest.mark.gpu
N, M = 700, 64
PARAMS = ("_features_dc", "_features_rest", "_scaling", "_opacity", "_rotation")


def _warp(dynamic_half=False):
    """A ``ControlNodeWarp`` of M nodes whose node Gaussians are all N points of a cloud (the state before the sampling step),
    every appearance parameter random; ``dynamic_half``: the motion mask of the odd points below 0.5."""
    from riggs_amd.control_nodes import ControlNodeWarp
    from riggs_amd.node_network import DeformNetwork
    cfg = NR.CONFIGS["w64"]
    net = DeformNetwork(D=8, W=64, is_blender=cfg["is_blender"], local_frame=cfg["local_frame"], pred_opacity=cfg["pred_opacity"],
                        max_d_scale=cfg["max_d_scale"])
    net.load_state_dict({k: v.float() for k, v in NR.integer_params(cfg).items()})
    cn = ControlNodeWarp(node_num=M, K=3, hyper_dim=2, local_frame=True, network=net).cuda()
    g = torch.Generator().manual_seed(41)
    pcl = (torch.rand(N, 3, generator=g) * 0.8 - 0.4).cuda()
    cn.init(_Opt(), pcl, force_init=True, force_gs_keep_all=True, as_gs_force_with_motion_mask=True, start=3)
    gs = cn.as_gaussians
    assert gs.get_xyz.shape == (N, 3) and cn.node_num == M and gs.with_motion_mask
    with torch.no_grad():
        for name in PARAMS:
            p = getattr(gs, name)
            p.copy_(torch.randn(p.shape, generator=g).cuda())
        gs.feature[:, -1] = 2.0 * torch.randn(N, generator=g).abs().cuda() + 0.1
        if dynamic_half:
            gs.feature[1::2, -1] *= -1
    return cn, gs


def _statements(cn, gs, time_num=16):
    """train_gui.py:1349-1357 on the library's query_network"""
    with torch.no_grad():
        t_samp = torch.linspace(0, 1, time_num).cuda()
        x = gs.get_xyz.detach()
        trans_samp = []
        for i in range(time_num):
            time_input = t_samp[i:i + 1, None].expand_as(x[..., :1])
            trans_samp.append(cn.query_network(x=x, t=time_input)["d_xyz"] * gs.motion_mask)
        trans_samp = torch.stack(trans_samp, dim=1)
        return (trans_samp + gs.get_xyz[:, None]).reshape([gs.get_xyz.shape[0], -1])


def test_hyper_trajectories_are_the_reference_statements():
    cn, gs = _warp()
    hyper = cn.hyper_trajectories(gs.get_xyz, gs.motion_mask)
    assert hyper.shape == (N, 48) and not hyper.requires_grad
    assert torch.equal(hyper, _statements(cn, gs))
    moved = (hyper.reshape(N, 16, 3) - gs.get_xyz.detach()[:, None]).abs().amax(dim=(0, 2))
    assert float(moved.min()) > 1e-4  # the network moves the points at every time: the rows are not the positions repeated


def test_samp_hyper_picks_by_trajectory_and_gathers_the_picked_rows():
    from riggs_amd.fps import farthest_point_sample_rows
    results = []
    for _ in range(2):
        cn, gs = _warp()
        old = {name: getattr(gs, name).detach().clone() for name in PARAMS + ("_xyz",)}
        hyper = _statements(cn, gs)
        idx = cn.downsample(_Opt(), "samp_hyper", start=17)
        want = farthest_point_sample_rows(hyper[None], M, start=[17])[0]
        assert idx.dtype == torch.int64 and torch.equal(idx, want) and int(idx[0]) == 17 and len(set(idx.tolist())) == M
        new = cn.as_gaussians
        assert new is not gs and new.get_xyz.shape == (M, 3) and new.optimizer is not None
        assert torch.equal(cn.nodes[:, :3].detach(), old["_xyz"][idx]) and torch.equal(new.get_xyz.detach(), old["_xyz"][idx])
        for name in PARAMS:
            p = getattr(new, name)
            assert isinstance(p, torch.nn.Parameter) and torch.equal(p.detach(), old[name][idx]), name
        held = {id(p) for grp in new.optimizer.param_groups for p in grp["params"]}
        assert {id(getattr(new, name)) for name in PARAMS} <= held
        results.append(idx)
    assert torch.equal(results[0], results[1])  # the same start: the same nodes


def test_dynamic_mask_picks_from_the_dynamic_half():
    from riggs_amd.fps import farthest_point_sample_rows
    cn, gs = _warp(dynamic_half=True)
    mask = gs.motion_mask[..., 0] > .5
    assert int(mask.sum()) == N // 2
    old_dc, old_xyz = gs._features_dc.detach().clone(), gs.get_xyz.detach().clone()
    hyper = _statements(cn, gs)
    idx = cn.downsample(_Opt(), "samp_hyper", with_dynamic_mask=True, start=2)
    assert torch.equal(idx, farthest_point_sample_rows(hyper[mask][None], M, start=[2])[0])
    picked = torch.nonzero(mask)[:, 0][idx]
    assert bool((picked % 2 == 0).all())
    assert torch.equal(cn.as_gaussians._features_dc.detach(), old_dc[picked]) and torch.equal(cn.nodes[:, :3].detach(), old_xyz[picked])


def test_direct_keeps_every_node_gaussian_and_shares_the_storage():
    cn, gs = _warp()
    assert cn.downsample(_Opt(), "direct") is None
    new = cn.as_gaussians
    assert cn.node_num == N and new is not gs and new.get_xyz.shape == (N, 3)
    assert torch.equal(cn.nodes[:, :3].detach(), gs.get_xyz.detach())
    for name in PARAMS:
        assert getattr(new, name).data_ptr() == getattr(gs, name).data_ptr(), name


def test_fewer_masked_points_than_nodes_are_refused():
    from riggs_amd import _lib as L
    cn, gs = _warp()
    with torch.no_grad():
        gs.feature[40:, -1] = -3.0
    with pytest.raises(L.RiggsHipError, match="40 .*64"):
        cn.downsample(_Opt(), "samp_hyper", with_dynamic_mask=True)
    with pytest.raises(L.RiggsHipError):
        cn.downsample(_Opt(), "nearest")
