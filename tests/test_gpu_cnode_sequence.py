"""GPU: stage-1 playback — ``ControlNodeWarp.deform_sequence`` (csrc/cnode.hip: cnode_sequence_kernel), ``render_time_sequence``
and ``precompute_deformations(sequence_chunk=)`` against the float64 oracle on the kernel's own lists (tests/cnode_sequence_ref.py),
the per-frame module, and the reference's goldens (tests/golden/cnodeseq_*.npz)."""
import numpy as np
import pytest
import torch

from tests import cnode_sequence_ref as SR

pytestmark = pytest.mark.gpu

OUT3 = ("d_xyz", "d_rotation", "d_scaling")
TOL = 1e-5  # the bar of tests/test_gpu_cnode.py: 1e-5 max(1, |ref|)


def _close(got, ref, what):
    got, ref = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got), np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.size:
        err = np.abs(got.astype(np.float64) - ref).max()
        assert err <= TOL * max(1.0, np.abs(ref).max()), (what, err)


def _frames(which, M, flags):
    from riggs_amd.control_nodes import sequence_pass_frames
    F = sequence_pass_frames(M, flags)
    assert F >= 1
    return {"1": 1, "2": 2, "F": F, "F+1": F + 1, "2F+1": 2 * F + 1}[which]


# N: one thread, a workgroup's tail, several workgroups; (M, K): K = M, the largest K, the rest; hyper 0 / 2 / 11; the four flag
# combinations; a per-Gaussian mask or none; node weights on / off; T = 1, 2, F, F + 1, 2 F + 1 frames (F: frames per pass)
@pytest.mark.parametrize("N,M,K,hyper,local,res,use_mask,nw,frames", [
    (1, 5, 5, 0, False, False, True, True, "1"),
    (257, 5, 5, 2, True, False, False, True, "2"),
    (257, 40, 8, 11, True, True, True, False, "F"),
    (1027, 40, 8, 0, False, True, False, True, "F+1"),
    (1027, 64, 3, 2, True, True, True, True, "2F+1"),
    (1027, 512, 3, 11, True, False, True, False, "2F+1"),
    (257, 512, 3, 2, False, False, False, True, "F+1"),
    (1, 64, 3, 11, True, True, True, True, "F"),
    (1027, 64, 3, 0, False, True, True, False, "1"),
    (257, 64, 3, 2, True, True, False, False, "2"),
    (1027, 5, 5, 11, False, False, True, True, "F"),
    (1, 512, 3, 0, True, False, False, False, "2F+1"),
])
def test_sequence_against_the_oracle_on_the_kernels_lists(N, M, K, hyper, local, res, use_mask, nw, frames):
    from riggs_amd.control_nodes import control_node_blend, control_node_blend_sequence
    from tests import cnode_f64_ref as R
    T = _frames(frames, M, (1 if local else 0) | (2 if res else 0))
    g = torch.Generator().manual_seed(1000 * N + M + T)
    x = torch.randn(N, 3, generator=g) * 0.5
    nodes = torch.cat([x[torch.randint(0, N, (M,), generator=g)] + 0.05 * torch.randn(M, 3, generator=g),
                       1e-2 + 0.02 * torch.randn(M, hyper, generator=g)], -1)
    feature = 0.02 * torch.randn(N, hyper + 1, generator=g) if hyper else None
    mask = torch.rand(N, 1, generator=g) if use_mask else None
    radius = np.log(0.15) + 0.3 * torch.randn(M, generator=g)
    weight = 0.5 * torch.randn(M, 1, generator=g) if nw else None
    attrs = {"d_xyz": 0.1 * torch.randn(T, M, 3, generator=g), "d_rotation": 0.2 * torch.randn(T, M, 4, generator=g),
             "d_scaling": 0.05 * torch.randn(T, M, 3, generator=g), "local_rotation": 0.3 * torch.randn(T, M, 4, generator=g)}
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731
    cfg = dict(K=K, hyper_dim=hyper, local_frame=local, d_rot_as_res=res)
    c_attrs = {k: v.cuda().requires_grad_(True) for k, v in attrs.items()}  # (a graph on the inputs must not reach the outputs)
    out = control_node_blend_sequence(cu(x), cu(feature), cu(mask), cu(nodes).requires_grad_(True), cu(radius), cu(weight), c_attrs, **cfg)
    assert out["d_xyz"].shape == (T, N, 3) and out["d_rotation"].shape == (T, N, 4) and out["d_scaling"].shape == (T, N, 3)
    assert out["nn_idx"].shape == (N, K) and out["nn_idx"].dtype == torch.int32
    for k in OUT3 + ("nn_idx", "nn_weight", "nn_dist"):
        assert not out[k].requires_grad and out[k].grad_fn is None, k
    for k in OUT3:
        assert out[k][T - 1].is_contiguous() and bool(torch.isfinite(out[k][T - 1]).all()), k
    # the lists: those of the per-frame entry, bit for bit, and admitted by the float64 selection rule
    one = control_node_blend(cu(x), cu(feature), cu(mask), cu(nodes), cu(radius), cu(weight), {k: v[0].cuda() for k, v in attrs.items()}, **cfg)
    assert torch.equal(out["nn_idx"], one["nn_idx"]) and torch.equal(out["nn_dist"], one["nn_dist"])
    assert R.selection_violations(x, feature, nodes, hyper, out["nn_idx"].cpu(), out["nn_dist"].cpu()) == 0
    # every output of every frame against the float64 oracle on those lists: no rows left out
    npy = lambda t: None if t is None else t.numpy()  # noqa: E731
    m_np = npy(mask) if mask is not None else np.ones((N, 1), np.float32)
    ref = SR.forward_sequence(x.numpy(), npy(feature), m_np, nodes.numpy(), radius.numpy(), npy(weight), {k: v.numpy() for k, v in attrs.items()},
                              nn_idx=out["nn_idx"].cpu().numpy(), **cfg)
    for k in OUT3 + ("nn_weight", "nn_dist"):
        _close(out[k], ref[k], k)


class _TorchNodeNet(torch.nn.Module):
    """A small torch node network with every head (nodes, t -> per-node attributes), opacity and colour included."""

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Linear(4, 32), torch.nn.Tanh(), torch.nn.Linear(32, 18))

    def forward(self, x, t, **kw):
        o = self.body(torch.cat([x, t], -1)) * torch.tensor([.05] * 3 + [.1] * 4 + [.02] * 3 + [.2] * 4 + [.3] * 4, device=x.device)
        return {"d_xyz": o[:, :3], "d_rotation": o[:, 3:7], "d_scaling": o[:, 7:10], "local_rotation": o[:, 10:14], "hidden": None,
                "d_opacity": o[:, 14:15], "d_color": o[:, 15:18]}


def _warp(network, N, M, seed, hyper=2, **kw):
    from riggs_amd.control_nodes import ControlNodeWarp
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, 3, generator=g) - 0.5).cuda()
    cn = ControlNodeWarp(node_num=M, K=3, hyper_dim=hyper, network=network, **kw).cuda()
    with torch.no_grad():
        cn.nodes.copy_(torch.cat([x[torch.randperm(N, generator=g)[:M].cuda()], 1e-2 + 0.02 * torch.randn(M, cn.hyper_dim, generator=g).cuda()], -1))
        if not cn.skinning:
            cn._node_radius.fill_(float(np.log(0.15)))
            cn._node_weight.copy_(0.3 * torch.randn(M, 1, generator=g))
    cn.inited.data = torch.ones_like(cn.inited)
    feature = torch.cat([0.02 * torch.randn(N, hyper, generator=g), 2.0 + torch.randn(N, 1, generator=g)], -1).cuda()
    return cn, x, feature, torch.sigmoid(feature[:, -1:])


def _loop(cn, x, times, feature, mask):
    with torch.no_grad():
        return [cn(x, t, feature, mask) for t in times]


def _agree(seq, per, keys):
    for f, p in enumerate(per):
        for k in keys:
            _close(seq[k][f], p[k], (k, f))


@pytest.mark.parametrize("which", ["mlp", "hash", "pred"])
def test_deform_sequence_agrees_with_a_loop_of_forward(which):
    """N = 1027, M = 64, T = 5 on the same module.  (The node network may pick another workgroup shape for T M rows than for M
    rows: 1e-5, not bit equality.)"""
    N, M, T = 1027, 64, 5
    torch.manual_seed(31)
    kw = dict(local_frame=True)
    if which == "mlp":
        from riggs_amd.node_network import DeformNetwork
        net = DeformNetwork(D=8, W=64, is_blender=True, local_frame=True)
    elif which == "hash":
        from riggs_amd.hash_network import HashDeformNetwork
        net = HashDeformNetwork(hidden_dim=64, local_frame=True)
        with torch.no_grad():  # (the trunk's last layer is drawn at 1e-5: lift it so that the frames differ visibly)
            net.mlp.layers[-1].weight.normal_(0, 0.1)
            net.hashgrid.encoding.params.uniform_(-0.5, 0.5)
        kw["use_hash"] = True
    else:
        net, kw = _TorchNodeNet(), dict(local_frame=False, d_rot_as_res=False, pred_opacity=True, pred_color=True)
    cn, x, feature, mask = _warp(net, N, M, 77, **kw)
    cn.train()
    cn.reg_loss = 123.0
    times = torch.linspace(0.05, 0.95, T, device="cuda")
    seq = cn.deform_sequence(x, times, feature, mask)
    assert cn.reg_loss == 123.0 and cn.training  # left alone
    assert torch.equal(seq["times"], times) and seq["d_nodes"].shape == (T, M, 3) and seq["d_xyz"].shape == (T, N, 3)
    assert all(not v.requires_grad for v in seq.values() if torch.is_tensor(v))
    per = _loop(cn, x, times, feature, mask)
    keys = OUT3 + ("d_nodes",) + (("d_opacity", "d_color") if which == "pred" else ())
    _agree(seq, per, keys)
    if which == "pred":
        assert seq["d_opacity"].shape == (T, N, 1) and seq["d_color"].shape == (T, N, 3)
    else:
        assert seq["d_opacity"] is None and seq["d_color"] is None
    assert torch.equal(seq["nn_idx"], per[0]["nn_idx"]) and torch.equal(seq["nn_dist"], per[0]["nn_dist"])
    assert float((seq["d_nodes"][0] - seq["d_nodes"][T - 1]).abs().max()) > 0  # time moves the nodes
    # animation_d_values replace the network's attributes, per frame
    over = {"d_xyz": 0.1 * torch.randn(T, M, 3, device="cuda")}
    seq2 = cn.deform_sequence(x, times, feature, mask, animation_d_values=over)
    with torch.no_grad():
        one = cn(x, times[3], feature, mask, animation_d_values={"d_xyz": over["d_xyz"][3]})
    _close(seq2["d_xyz"][3], one["d_xyz"], "override")
    _close(seq2["d_nodes"][3], one["d_nodes"], "override nodes")


def test_deform_sequence_with_skinning_agrees_with_the_loop():
    N, M, T = 257, 16, 3
    torch.manual_seed(5)
    cn, x, _, _ = _warp(_TorchNodeNet(), N, M, 78, skinning=True, d_rot_as_res=False, pred_opacity=True, pred_color=True)
    feature = torch.randn(N, M, device="cuda")
    mask = torch.rand(N, 1, device="cuda")
    times = torch.tensor([0.1, 0.5, 0.9], device="cuda")
    seq = cn.deform_sequence(x, times, feature, mask)
    per = _loop(cn, x, times, feature, mask)
    _agree(seq, per, OUT3 + ("d_nodes", "d_opacity", "d_color"))
    assert seq["d_xyz"].shape == (T, N, 3) and seq["nn_weight"].shape == (N, M) and not seq["d_xyz"].requires_grad


@pytest.mark.parametrize("name", SR.GOLDENS)
def test_deform_sequence_matches_the_reference_golden(name):
    from riggs_amd.control_nodes import ControlNodeWarp
    z = SR.golden(name)
    cu = lambda a: torch.from_numpy(np.asarray(a)).cuda()  # noqa: E731
    pred, h = bool(z["pred"]), int(z["hyper_dim"])
    cn = ControlNodeWarp(node_num=z["nodes"].shape[0], K=int(z["K"]), with_node_weight=True, local_frame=bool(z["local_frame"]),
                         d_rot_as_res=bool(z["d_rot_as_res"]), hyper_dim=h, pred_opacity=pred, pred_color=pred).cuda()
    cn.nodes.data, cn._node_radius.data, cn._node_weight.data = cu(z["nodes"]), cu(z["_node_radius"]), cu(z["_node_weight"])
    attrs = {k[5:]: cu(z[k]) for k in z.files if k.startswith("attr_")}
    out = cn.deform_sequence(cu(z["x"]), cu(z["times"]), cu(z["feature"]) if h else None, cu(z["motion_mask"]), animation_d_values=attrs)
    assert torch.equal(out["nn_idx"].cpu(), torch.from_numpy(z["nn_idx"]))  # every row: the maker left no near-tie
    assert np.abs(out["nn_weight"].cpu().numpy() - z["nn_weight"]).max() < 2e-6
    keys = [k[4:] for k in z.files if k.startswith("out_")]
    assert set(keys) == set(OUT3 + ("d_nodes",) + (("d_opacity", "d_color") if pred else ()))
    for k in keys:
        _close(out[k], z["out_" + k], k)


def test_edge_cases():
    from riggs_amd import _lib as L
    cn, x, feature, mask = _warp(_TorchNodeNet(), 100, 16, 3, local_frame=True, pred_opacity=True, pred_color=True)
    t3 = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    out = cn.deform_sequence(x, torch.zeros(0, device="cuda"), feature, mask)  # T = 0
    shapes = {"d_xyz": (0, 100, 3), "d_rotation": (0, 100, 4), "d_scaling": (0, 100, 3), "d_nodes": (0, 16, 3), "d_opacity": (0, 100, 1),
              "d_color": (0, 100, 3), "nn_idx": (100, 3), "nn_weight": (100, 3), "nn_dist": (100, 3), "times": (0,)}
    assert {k: tuple(out[k].shape) for k in shapes} == shapes
    out = cn.deform_sequence(x[:0], t3, feature[:0], mask[:0])  # N = 0
    shapes = {"d_xyz": (3, 0, 3), "d_rotation": (3, 0, 4), "d_scaling": (3, 0, 3), "d_nodes": (3, 16, 3), "d_opacity": (3, 0, 1),
              "d_color": (3, 0, 3), "nn_idx": (0, 3), "nn_weight": (0, 3), "nn_dist": (0, 3), "times": (3,)}
    assert {k: tuple(out[k].shape) for k in shapes} == shapes
    with pytest.raises(NotImplementedError):
        cn.deform_sequence(x, t3, feature, mask, node_trans_bias=torch.zeros(16, 3, device="cuda"))
    with pytest.raises(ValueError):
        cn.deform_sequence(x, t3[:, None], feature, mask)
    with pytest.raises(ValueError):
        cn.deform_sequence(x, torch.tensor(0.3, device="cuda"), feature, mask)
    for bad in (torch.zeros(16, 3), torch.zeros(2, 16, 3), torch.zeros(3, 15, 3), torch.zeros(3, 16, 4)):
        with pytest.raises(ValueError):
            cn.deform_sequence(x, t3, feature, mask, animation_d_values={"d_xyz": bad.cuda()})
    # the C entry: no launch and NULL per-Gaussian pointers for an empty call; the limits of riggs_cnode_forward
    lib = L.lib()
    null = [None] * 17
    assert lib.riggs_cnode_sequence_forward(0, 16, 3, 3, 0, 0, 3, 0, *null) == 0
    assert lib.riggs_cnode_sequence_forward(100, 16, 0, 3, 0, 0, 3, 0, *null) == 0
    assert lib.riggs_cnode_sequence_forward(100, 16, 3, 9, 0, 0, 3, 0, *null) != 0  # K > 8
    assert lib.riggs_cnode_sequence_forward(100, 16, -1, 3, 0, 0, 3, 0, *null) != 0


class _Pipe:
    convert_SHs_python = compute_cov3D_python = debug = False


def _render_stage(N=1027, M=64):
    from riggs_amd import synth
    from riggs_amd.gaussian_model import GaussianModel
    sc = synth.make_scene(N, 8, 4321, scale=0.03)
    gm = GaussianModel.from_tensors(sc["xyz"], sc["features_dc"], sc["features_rest"], sc["scaling"], sc["rotation"], sc["opacity"])
    torch.manual_seed(9)
    cn, _, feature, _ = _warp(_TorchNodeNet(), N, M, 12, local_frame=True)
    with torch.no_grad():
        cn.nodes[:, :3] = gm.get_xyz[torch.randperm(N)[:M].cuda()]
    gm.fea_dim, gm.with_motion_mask, gm.feature = 3, True, torch.nn.Parameter(feature)
    cams = [synth.look_at_camera(64, 64, azimuth_deg=20.0 + 15.0 * f).to("cuda") for f in range(3)]
    return gm, cn, cams, torch.tensor([0.1, 0.3, 0.7], device="cuda")


@pytest.mark.parametrize("moving_camera", [False, True])
def test_render_time_sequence_is_render_on_the_frames_of_deform_sequence(moving_camera):
    from riggs_amd import playback as PB
    from riggs_amd.render import render
    gm, cn, cams, bg = _render_stage()
    times = torch.tensor([0.1, 0.45, 0.8], device="cuda")

    class Model:  # a model holding the warp as .deform
        deform = cn
    got = list(PB.render_time_sequence(cams if moving_camera else cams[0], gm, Model, _Pipe, bg, times, chunk=2))
    assert len(got) == 3
    seq = cn.deform_sequence(gm.get_xyz.detach(), times, gm.feature, gm.motion_mask)
    for f, (pkg, d_nodes) in enumerate(got):
        with torch.no_grad():
            want = render(cams[f] if moving_camera else cams[0], gm, _Pipe, bg, seq["d_xyz"][f], seq["d_rotation"][f], seq["d_scaling"][f],
                          d_opacity=None, d_color=None, d_rot_as_res=cn.d_rot_as_res)
        assert pkg["render"].shape == (3, 64, 64) and float(pkg["alpha"].max()) > 0.5
        for k in ("render", "alpha", "depth", "radii"):
            assert torch.equal(pkg[k], want[k]), (k, f)
        assert torch.equal(d_nodes, seq["d_nodes"][f])
    assert not torch.equal(got[0][0]["render"], got[2][0]["render"])  # the frames move
    with pytest.raises(ValueError):
        next(PB.render_time_sequence(cams[:2], gm, cn, _Pipe, bg, times))
    with pytest.raises(ValueError):
        next(PB.render_time_sequence(cams[0], gm, cn, _Pipe, bg, times[None]))
    # isotropic Gaussians: the rotation and scale residuals are zeroed before the render
    gm.use_isotropic_gs = True
    pkg, _ = next(PB.render_time_sequence(cams[0], gm, cn, _Pipe, bg, times[:1]))
    with torch.no_grad():
        z = torch.zeros_like
        want = render(cams[0], gm, _Pipe, bg, seq["d_xyz"][0], z(seq["d_rotation"][0]), z(seq["d_scaling"][0]), d_rot_as_res=cn.d_rot_as_res)
    assert torch.equal(pkg["render"], want["render"])


def test_precompute_deformations_through_the_sequence():
    """A seeded synthetic stage 1 whose discrete choices — the template frame, the tree — are far from a tie: checked on the CPU
    (the nodes' tracks perturbed by 1e-5 relative, twenty draws: the same template frame and tree every time)."""
    from riggs_amd import skeleton_init as SI
    from tests import skeleton_init_ref as R
    fids = torch.tensor([0.8, 0.0, 0.2, 1.0, 0.4, 0.6, 0.5])
    coverage = torch.tensor([5.0, 9.0, 1.0, 2.0, 3.0, 4.0, 6.0])
    res = []
    for chunk in (None, 3):
        warp, gm = R.stage1_scene()
        xyz0 = gm.get_xyz.detach().clone()
        info, tree, offsets = SI.precompute_deformations(warp, gm, fids, coverage=coverage, sequence_chunk=chunk)
        res.append((info, tree, offsets, gm.get_xyz.detach() - xyz0))
    (a, ta, oa, sa), (b, tb, ob, sb) = res
    assert b["d_xyz"].shape == (7, 500, 3) and b["d_nodes"].shape == (7, 64, 3)
    assert ta["template_idx"] == tb["template_idx"]
    assert torch.equal(ta["parent_indices"], tb["parent_indices"]) and torch.equal(ta["joint_node_indices"], tb["joint_node_indices"])
    for k in ("d_xyz", "d_nodes", "d_rotation", "d_scaling", "d_joints"):
        _close(b[k], a[k], k)
    _close(ob, oa, "template offsets")
    _close(sb, sa, "the Gaussians' shift")
    assert float(b["d_xyz"][tb["template_idx"]].abs().max()) == 0.0
