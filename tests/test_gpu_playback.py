"""-m gpu: pose-track playback (riggs_amd/playback.py; csrc/playback.hip: riggs_pose_slerp; csrc/deform.hip:
riggs_lbs_sequence_forward, riggs_skinning_colors).

References: goldens captured from the reference (tests/golden/playback_*.npz), the CPU restatement tests/playback_ref.py (a loop
of the pinned oracle's deform_by_pose) on seeded riggs_amd.synth scenes, and — for the top-K selection — this library's own
per-frame deform_by_pose, which shares the selection code and is pinned to the reference elsewhere.

Bounds: 1e-5 relative for pose-level quantities (interpolated poses, d_nodes), U.REL_TOL = 1e-4 for per-Gaussian outputs — the
suite's bars; unit norms within 1e-6; bit equality where a value is gathered or the same calls are issued (segment colours, node
colours, render_sequence's frames, the per-frame path before and after).

One golden is not compared on every row: playback_colors_tree24_n300_k3 (K = 3).  Bones that share a joint give distances that
tie up to rounding, and torch.topk — the reference's selection — leaves the order of ties undefined, so the reference pins only the
rows whose K-th and (K+1)-th distances are separated by more than 1e-5 relative (the rule of tests/test_gpu_deform.py:42-51; the
test asserts that more than 80 % of the rows are kept); every row is compared against this library's own nn_idx / nn_weight.

Shapes are the smallest that take every path: N in {1, 257, 1027} (one thread, a workgroup's tail, several workgroups);
J in {2, 24, 64, 65, 200} (one bone, the wave's last lane, the first joint of the 128- and of the 256-joint form); M in
{1, F, F + 1, 2 F + 1} for the pass F the library reports for that joint count (a partial pass, a full one, a pass of one
frame after a full one, two full ones and a frame)."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import deform_ref as O  # noqa: E402
from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import playback as PB  # noqa: E402
from riggs_amd import synth  # noqa: E402
from riggs_amd.gaussian_model import GaussianModel  # noqa: E402
from riggs_amd.render import render  # noqa: E402
from riggs_amd.skeleton import SkeletonWarp  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import playback_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POSE_TOL = 1e-5


def T(a):
    return torch.from_numpy(np.asarray(a))


def npy(t):
    return t.detach().cpu().numpy()


def gold(pat):
    out = sorted(glob.glob(os.path.join(GOLD, pat)))
    assert out, pat
    return out


def warp(joints, parents, rho, K, weight_mlp=False, offsets=False, seed=0):
    torch.manual_seed(seed)
    sw = SkeletonWarp(joints=joints, parent_indices=parents, K=K, hyper_dim=8, use_skinning_weight_mlp=weight_mlp,
                      use_template_offsets=offsets).cuda()
    sw._node_radius.data = rho.clone().cuda()
    if offsets:  # (the reference initialises this head at std 1e-5: make the offsets visible)
        with torch.no_grad():
            sw.detail_net.gaussian_warp.weight.mul_(2000.0)
            sw.detail_net.gaussian_warp.bias.add_(0.01)
    return sw


def track(M, J, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([1.0, 0, 0, 0]) + 0.3 * torch.randn(M, J, 4, generator=g), 0.02 * torch.randn(M, 3, generator=g)


def unit_norms(q, what):
    err = float((q.double().norm(dim=-1) - 1).abs().max())
    assert err <= 1e-6, "%s: |q| off by %.3g" % (what, err)


# ------------------------------------------------------------------------------------------------ key poses -> a track
@pytest.mark.parametrize("path", gold("playback_slerp_*.npz"), ids=lambda p: os.path.basename(p)[:-4])
def test_slerp_batch_against_the_reference(path):
    g = np.load(path)
    out = PB.slerp_batch(T(g["q0"]).cuda(), T(g["q1"]).cuda(), T(g["t"]).cuda())
    assert out.shape == g["out"].shape and bool(torch.isfinite(out).all())
    U.assert_close(npy(out), g["out"], "slerp_batch", POSE_TOL)
    unit_norms(out, "slerp_batch")


def test_run_interpolation_against_the_reference():
    g = np.load(os.path.join(GOLD, "playback_interp_p3_j24_f7.npz"))
    keys = [{"local_rotation2": T(g["key_rot"][i]).cuda(), "global_trans": T(g["key_trans"][i]).cuda()} for i in range(3)]
    out = PB.run_interpolation(keys, "cuda", num_frames=int(g["num_frames"]))
    assert out["num"] == 14 and out["local_rotation"] is out["local_rotation2"] and out["local_rotation"].shape == (14, 24, 4)
    assert bool(torch.isfinite(out["local_rotation"]).all()) and bool(torch.isfinite(out["global_trans"]).all())
    U.assert_close(npy(out["local_rotation"]), g["local_rotation"], "interpolated rotations", POSE_TOL)
    U.assert_close(npy(out["global_trans"]), g["global_trans"], "interpolated translations", POSE_TOL)
    unit_norms(out["local_rotation"], "run_interpolation")
    # the editor's name for the key poses gives the same track
    out2 = PB.run_interpolation([{"local_rotation": k["local_rotation2"], "global_trans": k["global_trans"]} for k in keys], "cuda", 7)
    assert torch.equal(out2["local_rotation"], out["local_rotation"]) and torch.equal(out2["global_trans"], out["global_trans"])
    assert PB.run_interpolation(keys[:1], "cuda") is None


# ------------------------------------------------------------------------------------------------ a track over one cloud
def check_sequence(out, ref, N, M, J, what):
    assert out["d_xyz"].shape == (M, N, 3) and out["d_rotation"].shape == (M, N, 4) and out["d_nodes"].shape == (M, J, 3)
    assert out["d_scaling"].shape == (N, 3) and float(out["d_scaling"].abs().max()) == 0.0
    assert out["local_rotation"].shape == (M, J, 4)
    for k in ("d_xyz", "d_rotation", "d_nodes"):
        assert not out[k].requires_grad and out[k].grad_fn is None and out[k][M - 1].is_contiguous()
        assert bool(torch.isfinite(out[k]).all()), k
    U.assert_close(npy(out["d_xyz"]), npy(ref["d_xyz"]), what + " d_xyz", U.REL_TOL)
    U.assert_close(npy(out["d_rotation"]), npy(ref["d_rotation"]), what + " d_rotation", U.REL_TOL)
    U.assert_close(npy(out["d_nodes"]), npy(ref["d_nodes"]), what + " d_nodes", POSE_TOL)


@pytest.mark.parametrize("path", gold("playback_seq_*.npz"), ids=lambda p: os.path.basename(p)[:-4])
def test_deform_sequence_against_the_reference(path):
    g = np.load(path)
    K, N, J, M = int(g["K"]), g["x"].shape[0], g["joints"].shape[0], g["local_rotation"].shape[0]
    sw = warp(T(g["joints"]), T(g["parents"]), T(g["node_radius_log"]), K)
    keys = [{"local_rotation2": T(g["key_rot"][i]).cuda(), "global_trans": T(g["key_trans"][i]).cuda()} for i in range(2)]
    poses = PB.run_interpolation(keys, "cuda", num_frames=int(g["num_frames"]))  # what the reference's callers hand over
    out = sw.deform_sequence(T(g["x"]).cuda(), poses, T(g["motion_mask"]).cuda())
    check_sequence(out, {k: T(g[k]) for k in ("d_xyz", "d_rotation", "d_nodes")}, N, M, J, os.path.basename(path)[:-4])


# (N, J, K, which M, mask, global_trans, chain)
SWEEP = [
    (1027, 24, -1, "1", "none", "M3", False), (1027, 24, -1, "F", "tensor", "M13", False),
    (1027, 24, -1, "F+1", "scalar", "13", False), (1027, 24, -1, "2F+1", "tensor", "M3", False),
    (1, 24, -1, "F+1", "tensor", "M3", False), (257, 2, -1, "F+1", "none", "M3", True), (257, 8, -1, "2F+1", "tensor", "list", True),
    (257, 64, -1, "2F+1", "tensor", "M3", False), (1027, 65, -1, "F", "none", "M3", False), (257, 65, -1, "2F+1", "tensor", "13", False),
    (257, 200, -1, "1", "tensor", "M3", False), (257, 200, -1, "F", "none", "M13", False), (1027, 200, -1, "F+1", "scalar", "M3", False),
    (257, 200, -1, "2F+1", "tensor", "M3", False),
    (1027, 24, 3, "2F+1", "tensor", "M3", False), (257, 24, 3, "F", "none", "13", False), (1, 24, 3, "1", "none", "M3", False),
    (257, 64, 3, "F+1", "tensor", "M3", False), (257, 65, 3, "2F+1", "tensor", "M3", False), (1027, 65, 3, "F", "none", "M3", False),
    (257, 200, 3, "1", "none", "M3", False), (257, 200, 3, "F+1", "tensor", "M13", False), (1027, 200, 3, "2F+1", "scalar", "M3", False),
]


def frames(which, J, K):
    F = PB.sequence_pass_frames(J, K)
    assert F >= 1 and F == (4 if J <= 128 else (1 if K > 0 else 2))
    return {"1": 1, "F": F, "F+1": F + 1, "2F+1": 2 * F + 1}[which]


def sweep_inputs(N, J, K, which, mask_kind, gt_kind, chain):
    M = frames(which, J, K)
    sc = synth.make_scene(N, J, 4000 + N + J, chain=chain)
    lr, gt = track(M, J, 77 + M)
    g = torch.Generator().manual_seed(N + 3 * J)
    rho = sc["node_radius"] + 0.3 * torch.randn(J, generator=g)
    mask_cpu = {"none": torch.ones(N, 1), "tensor": torch.sigmoid(torch.randn(N, 1, generator=g)), "scalar": torch.full((N, 1), 0.5)}[mask_kind]
    mask_arg = {"none": None, "tensor": mask_cpu.cuda(), "scalar": 0.5}[mask_kind]
    if gt_kind == "13":
        gt = gt[:1]
    lr_d, gt_d = lr.cuda(), gt.cuda()
    if gt_kind == "list":  # render_rig.py:278-303: a list of node_attrs
        poses = [{"local_rotation": lr_d[f], "global_trans": gt_d[f][None], "d_xyz": None} for f in range(M)]
    else:
        poses = {"local_rotation": lr_d, "global_trans": {"M3": gt_d, "M13": gt_d[:, None], "13": gt_d, "list": None}[gt_kind]}
    return M, sc, rho, lr, gt, mask_cpu, mask_arg, poses


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "n%d_j%d_k%d_m%s_%s_%s" % c[:6])
def test_deform_sequence_over_the_shapes(case):
    N, J, K = case[:3]
    M, sc, rho, lr, gt, mask_cpu, mask_arg, poses = sweep_inputs(*case)
    sw = warp(sc["joints"], sc["parents"], rho, K)
    x = sc["xyz"].cuda()
    out = sw.deform_sequence(x, poses, mask_arg)
    if K > 0:
        # top-K against the per-frame path of this library on EVERY row: the selection code is shared, so no tie is excluded
        per = [sw.deform_by_pose(x, {"local_rotation": lr[f].cuda(), "global_trans": gt[f if gt.shape[0] > 1 else 0].cuda()}, mask_arg)
               for f in range(M)]
        ref = {k: torch.stack([p[k].detach() for p in per]) for k in ("d_xyz", "d_rotation", "d_nodes")}
    else:
        ref = R.deform_sequence(sc["xyz"], sc["joints"], sc["parents"], rho, lr, gt, mask_cpu, K)
    check_sequence(out, ref, N, M, J, "sequence")


@pytest.mark.parametrize("J,K", [(24, -1), (24, 3), (200, -1)])
def test_deform_sequence_walks_several_passes_per_workgroup(J, K):
    """At the sizes above every pass gets a slice of gridDim.y to itself (two workgroups of Gaussians leave the device empty).  A
    track of more than 256 passes makes a workgroup walk two passes, and the last slice a single one: 300 passes and a frame over
    257 Gaussians.  The frames of a track are independent, so the track repeats nine poses and the reference is computed once."""
    N, P = 257, 9
    F = PB.sequence_pass_frames(J, K)
    M = 300 * F + 1
    sc = synth.make_scene(N, J, 4800 + J)
    lr9, gt9 = track(P, J, 21)
    mask = torch.sigmoid(torch.randn(N, 1, generator=torch.Generator().manual_seed(6)))
    sw = warp(sc["joints"], sc["parents"], sc["node_radius"], K)
    x = sc["xyz"].cuda()
    if K > 0:
        per = [sw.deform_by_pose(x, {"local_rotation": lr9[p].cuda(), "global_trans": gt9[p].cuda()}, mask.cuda()) for p in range(P)]
        ref9 = {k: torch.stack([d[k].detach().cpu() for d in per]) for k in ("d_xyz", "d_rotation", "d_nodes")}
    else:
        ref9 = R.deform_sequence(sc["xyz"], sc["joints"], sc["parents"], sc["node_radius"], lr9, gt9, mask, K)
    pick = torch.arange(M) % P
    out = sw.deform_sequence(x, {"local_rotation": lr9[pick].cuda(), "global_trans": gt9[pick].cuda()}, mask.cuda())
    check_sequence(out, {k: v[pick] for k, v in ref9.items()}, N, M, J, "long track")


def test_deform_sequence_with_the_weight_head_evaluates_it_once(monkeypatch):
    for J, N in ((24, 1027), (64, 257)):  # (23 bones: the rows go through the LDS tile; 63: read from global memory)
        sc = synth.make_scene(N, J, 4100 + J)
        sw = warp(sc["joints"], sc["parents"], sc["node_radius"], -1, weight_mlp=True, seed=J)
        M = frames("F+1", J, -1)
        lr, gt = track(M, J, 5)
        x = sc["xyz"].cuda()
        calls = []
        inner = sw._head_weight
        monkeypatch.setattr(sw, "_head_weight", lambda xx: (calls.append(1), inner(xx))[1])
        out = sw.deform_sequence(x, {"local_rotation": lr.cuda(), "global_trans": gt.cuda()}, None)
        assert len(calls) == 1
        with torch.no_grad():
            wm = sw.skinning_weight_mlp(x).cpu()
        ref = R.deform_sequence(sc["xyz"], sc["joints"], sc["parents"], sc["node_radius"], lr, gt, torch.ones(N, 1), -1, weight_offsets=wm)
        check_sequence(out, ref, N, M, J, "sequence + WeightMLP, J = %d" % J)


def test_deform_sequence_with_template_offsets():
    N, J = 257, 24
    sc = synth.make_scene(N, J, 4200)
    sw = warp(sc["joints"], sc["parents"], sc["node_radius"], -1, offsets=True, seed=3)
    M = frames("F+1", J, -1)
    lr, gt = track(M, J, 6)
    mask = torch.sigmoid(torch.randn(N, 1, generator=torch.Generator().manual_seed(1)))
    x = sc["xyz"].cuda()
    out = sw.deform_sequence(x, {"local_rotation": lr.cuda(), "global_trans": gt.cuda()}, mask.cuda())
    with torch.no_grad():
        offs = [sw.detail_net(x, lr[f].cuda().reshape(-1)[None].expand(N, -1)).cpu() for f in range(M)]
    assert float(torch.stack(offs).abs().max()) > 1e-3  # (the offsets are visible in the result)
    ref = R.deform_sequence(sc["xyz"], sc["joints"], sc["parents"], sc["node_radius"], lr, gt, mask, -1, template_offsets=offs)
    check_sequence(out, ref, N, M, J, "sequence + template offsets")


def test_top_k_with_the_weight_head_keeps_raising():
    sc = synth.make_scene(64, 8, 1)
    sw = warp(sc["joints"], sc["parents"], sc["node_radius"], 3, weight_mlp=True)
    lr, gt = track(2, 8, 1)
    with pytest.raises(NotImplementedError):
        sw.deform_sequence(sc["xyz"].cuda(), {"local_rotation": lr.cuda(), "global_trans": gt.cuda()}, None)
    with pytest.raises(NotImplementedError):
        sw.skinning_colors(sc["xyz"].cuda())
    with pytest.raises(L.RiggsHipError):
        warp(sc["joints"], sc["parents"], sc["node_radius"], -1).deform_sequence(
            sc["xyz"].cuda(), {"local_rotation": lr.cuda(), "global_trans": torch.zeros(3, 3).cuda()}, None)


def test_the_per_frame_path_is_what_it_was_after_a_sequence():
    N, J = 1027, 24
    sc = synth.make_scene(N, J, 4300)
    sw = warp(sc["joints"], sc["parents"], sc["node_radius"], -1, weight_mlp=True, offsets=True, seed=9)
    lr, gt = track(6, J, 8)
    x, mask = sc["xyz"].cuda(), torch.rand(N, 1, generator=torch.Generator().manual_seed(2)).cuda()
    pose = {"local_rotation": lr[2].cuda(), "global_trans": gt[2].cuda()}
    keys = ("d_xyz", "d_rotation", "d_nodes", "nn_weight", "nn_idx")
    before = sw.deform_by_pose(x, pose, mask)
    before = {k: before[k].detach().clone() for k in keys}
    seq = sw.deform_sequence(x, {"local_rotation": lr.cuda(), "global_trans": gt.cuda()}, mask)
    sw.skinning_colors(x)
    after = sw.deform_by_pose(x, pose, mask)
    for k in keys:
        assert torch.equal(before[k], after[k].detach()), k + " of deform_by_pose changed after deform_sequence"
    U.assert_close(npy(seq["d_xyz"][2]), npy(before["d_xyz"]), "frame 2 of the track vs deform_by_pose", U.REL_TOL)


# ------------------------------------------------------------------------------------------------ colours
def test_geometric_colours_on_the_device_are_the_references_bits():
    for path in gold("playback_colors_*.npz"):
        g = np.load(path)
        assert np.array_equal(npy(PB.get_geometric_color(T(g["joints"]).cuda())).view(np.uint32), g["node_colors"].view(np.uint32))
        assert np.array_equal(npy(PB.get_geometric_color(T(g["x"]).cuda())).view(np.uint32), g["point_colors"].view(np.uint32))
    for J in (8, 65, 200):
        joints = synth.make_scene(8, J, 4400 + J)["joints"]
        assert np.array_equal(npy(PB.get_geometric_color(joints.cuda())).view(np.uint32), R.get_geometric_color(joints).numpy().view(np.uint32))


@pytest.mark.parametrize("path", gold("playback_colors_*.npz"), ids=lambda p: os.path.basename(p)[:-4])
def test_skinning_colours_against_the_reference(path):
    g = np.load(path)
    sw = warp(T(g["joints"]), T(g["parents"]), T(g["node_radius_log"]), int(g["K"]))
    x = T(g["x"]).cuda()
    got = sw.skinning_colors(x, "blend")
    assert got.shape == (x.shape[0], 3)
    K, rows = int(g["K"]), np.ones(x.shape[0], bool)
    if K > 0:
        # bones that share a joint give distances that tie up to rounding, and torch.topk does not define the order of ties: as
        # in test_gpu_deform.py the reference pins the rows whose K-th and (K+1)-th distances are separated ...
        srt = np.sort(O.bone_dist2(T(g["x"]), T(g["joints"]), T(g["parents"])).numpy(), 1)
        rows = (srt[:, K] - srt[:, K - 1]) > 1e-5 * np.maximum(srt[:, K], 1e-12)
        assert rows.mean() > 0.8
    U.assert_close(npy(got)[rows], g["colors"][rows], "skinning_colors vs the reference", U.REL_TOL)
    # ... and EVERY row equals the colours through this library's own nn_idx / nn_weight (the same selection code)
    d = sw.deform_by_pose(x, {"local_rotation": torch.tensor([[1.0, 0, 0, 0]]).repeat(g["joints"].shape[0], 1).cuda(),
                              "global_trans": torch.zeros(3).cuda()}, None)
    own = PB.get_color_for_skinning_weights(x, d["nn_idx"], d["nn_weight"], sw.nodes.detach()[:, :3])
    U.assert_close(npy(got), npy(own), "skinning_colors vs the colours through nn_idx / nn_weight", U.REL_TOL)
    mirror = PB.get_color_for_skinning_weights(x, T(g["nn_idx"]).cuda(), T(g["nn_weight"]).cuda(), T(g["joints"]).cuda())
    U.assert_close(npy(mirror), g["colors"], "get_color_for_skinning_weights vs the reference", U.REL_TOL)


def test_skinning_colours_write_no_weight_matrix():
    """N = 20 000, J = 64: nn_weight alone would be N (J - 1) 4 B = 5.04 MB; the launch may allocate the (N, 3) output and the
    few J-row tensors of the node colours, so the peak stays below that matrix plus the output."""
    N, J = 20000, 64
    sc = synth.make_scene(N, J, 4500)
    sw = warp(sc["joints"], sc["parents"], sc["node_radius"], -1)
    x = sc["xyz"].cuda()
    d = sw.deform_by_pose(x, {"local_rotation": sc["local_rotation"].cuda(), "global_trans": sc["global_trans"].cuda()}, None)
    want = PB.get_color_for_skinning_weights(x, d["nn_idx"], d["nn_weight"], sw.nodes.detach()[:, :3])
    del d
    sw._joints(), sw._parents_dev(x.device)  # (cached per module, not per call)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = sw.skinning_colors(x, "blend")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < N * (J - 1) * 4 + N * 3 * 4, "skinning_colors allocated %d bytes" % peak
    assert peak < N * (J - 1) * 4  # (in fact far below the matrix itself)
    U.assert_close(npy(got), npy(want), "skinning_colors vs the colours through nn_idx / nn_weight", U.REL_TOL)
    sw3 = warp(sc["joints"], sc["parents"], sc["node_radius"], 3)
    d3 = sw3.deform_by_pose(x, {"local_rotation": sc["local_rotation"].cuda(), "global_trans": sc["global_trans"].cuda()}, None)
    want3 = PB.get_color_for_skinning_weights(x, d3["nn_idx"], d3["nn_weight"], sw3.nodes.detach()[:, :3])
    U.assert_close(npy(sw3.skinning_colors(x)), npy(want3), "skinning_colors, K = 3", U.REL_TOL)


@pytest.mark.parametrize("N,J,chain", [(1027, 24, False), (515, 65, False), (300, 8, True), (700, 200, False)])
def test_segment_colours_are_the_node_colour_of_the_largest_weight(N, J, chain):
    sc = synth.make_scene(N, J, 4600 + J, chain=chain)
    rho = sc["node_radius"] + 0.3 * torch.randn(J, generator=torch.Generator().manual_seed(J))
    w, _, idx = O.skin_weights(sc["xyz"], sc["joints"], sc["parents"], rho, -1)
    want, gap = R.segment_colors(idx, w, sc["joints"])
    keep = gap > 1e-4  # (closer than that, either bone may be the larger one in the kernel's arithmetic)
    assert float((~keep).float().mean()) <= 0.08
    got = warp(sc["joints"], sc["parents"], rho, -1).skinning_colors(sc["xyz"].cuda(), "segment").cpu()
    assert torch.equal(got[keep], want[keep])
    node_colors = R.get_geometric_color(sc["joints"])
    assert bool((got[:, None, :] == node_colors[None, 1:, :]).all(-1).any(-1).all())  # every row is SOME bone's colour, unchanged
    with pytest.raises(ValueError):
        warp(sc["joints"], sc["parents"], rho, -1).skinning_colors(sc["xyz"].cuda(), "nearest")


# ------------------------------------------------------------------------------------------------ render_sequence
class Pipe:
    convert_SHs_python = False
    compute_cov3D_python = False
    debug = False


@functools.lru_cache(maxsize=None)
def _stage():
    N, J, M, H, W = 2000, 24, 5, 64, 64
    sc = synth.make_scene(N, J, 4700, scale=0.03)
    gm = GaussianModel.from_tensors(sc["xyz"], sc["features_dc"], sc["features_rest"], sc["scaling"], sc["rotation"], sc["opacity"])
    sw = warp(sc["joints"], sc["parents"], sc["node_radius"], -1)
    lr, gt = track(M, J, 11)
    poses = {"local_rotation": lr.cuda(), "global_trans": gt.cuda()}
    mask = torch.sigmoid(torch.randn(N, 1, generator=torch.Generator().manual_seed(4))).cuda()
    cams = [synth.look_at_camera(H, W, azimuth_deg=30.0 + 12.0 * f).to("cuda") for f in range(M)]
    return dict(gm=gm, sw=sw, poses=poses, mask=mask, cams=cams, M=M, J=J, bg=torch.tensor([0.1, 0.3, 0.7], device="cuda"))


@pytest.mark.parametrize("moving_camera", [False, True])
def test_render_sequence_is_the_per_frame_calls(moving_camera):
    s = _stage()
    gm, sw, bg, M = s["gm"], s["sw"], s["bg"], s["M"]
    cam_arg = s["cams"] if moving_camera else s["cams"][0]
    got = []
    for pkg, skin, d_nodes in PB.render_sequence(cam_arg, gm, sw, Pipe, bg, s["poses"], motion_mask=s["mask"], skinning=True, chunk=2):
        assert pkg.lists is not None and skin is not None
        got.append((pkg["render"].detach().clone(), skin["render"].detach().clone(), pkg["alpha"].detach().clone(), d_nodes.clone()))
    assert len(got) == M
    x = gm.get_xyz.detach()
    seq = sw.deform_sequence(x, s["poses"], s["mask"])
    colours = sw.skinning_colors(x, "blend")
    zeros = torch.zeros(x.shape[0], 3, device="cuda")
    for f in range(M):
        cam = s["cams"][f] if moving_camera else s["cams"][0]
        main = render(cam, gm, Pipe, bg, seq["d_xyz"][f], seq["d_rotation"][f], zeros)
        assert torch.equal(got[f][0], main["render"].detach()), "frame %d" % f
        assert torch.equal(got[f][2], main["alpha"].detach()) and torch.equal(got[f][3], seq["d_nodes"][f])
        kept = render(cam, gm, Pipe, bg, seq["d_xyz"][f], seq["d_rotation"][f], zeros, keep_lists=True)
        skin = render(cam, gm, Pipe, bg, seq["d_xyz"][f], seq["d_rotation"][f], zeros, override_color=colours, lists=kept.lists)
        assert torch.equal(got[f][1], skin["render"].detach()), "skin frame %d" % f
        assert float((got[f][1] - got[f][0]).abs().max()) > 1e-3  # (the recolour is another image)
    if moving_camera:
        assert not torch.equal(got[0][0], got[1][0])
        with pytest.raises(ValueError):
            next(PB.render_sequence(s["cams"][:2], gm, sw, Pipe, bg, s["poses"]))
    # without skinning: no lists kept, nothing recoloured
    pkg, skin, _ = next(PB.render_sequence(s["cams"][0], gm, sw, Pipe, bg, s["poses"], motion_mask=s["mask"], chunk=3))
    assert skin is None and getattr(pkg, "lists", None) is None
    assert torch.equal(pkg["render"].detach(), render(s["cams"][0], gm, Pipe, bg, seq["d_xyz"][0], seq["d_rotation"][0], zeros)["render"].detach())


def test_render_sequence_evaluates_the_weight_head_once(monkeypatch):
    s = _stage()
    gm, bg, M = s["gm"], s["bg"], s["M"]
    sc = synth.make_scene(2000, s["J"], 4700, scale=0.03)
    sw = warp(sc["joints"], sc["parents"], sc["node_radius"], -1, weight_mlp=True, seed=12)
    calls = []
    inner = sw._head_weight
    monkeypatch.setattr(sw, "_head_weight", lambda xx: (calls.append(1), inner(xx))[1])
    frames_ = [(p["render"].detach().clone(), q["render"].detach().clone())
               for p, q, _ in PB.render_sequence(s["cams"][0], gm, sw, Pipe, bg, s["poses"], skinning=True, chunk=2)]
    assert len(frames_) == M and len(calls) == 1  # three chunks and the colours: one evaluation
    x = gm.get_xyz.detach()
    seq, colours = sw.deform_sequence(x, s["poses"], None), sw.skinning_colors(x)
    zeros = torch.zeros(x.shape[0], 3, device="cuda")
    kept = render(s["cams"][0], gm, Pipe, bg, seq["d_xyz"][3], seq["d_rotation"][3], zeros, keep_lists=True)
    assert torch.equal(frames_[3][0], kept["render"].detach())
    skin = render(s["cams"][0], gm, Pipe, bg, seq["d_xyz"][3], seq["d_rotation"][3], zeros, override_color=colours, lists=kept.lists)
    assert torch.equal(frames_[3][1], skin["render"].detach())
