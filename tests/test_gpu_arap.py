"""-m gpu: riggs_amd.arap (csrc/arap.hip) against tests/arap_ref.py — float64 (SVD rotation fit, float64 pseudo-inverse) is the
oracle, its float32 form (every operation rounded, the operator rounded to float32, a float32 SVD) the yardstick for rounding.

Bars.  PARITY per case and tensor: max(8 * e32, 1e-6), e32 = the float32 restatement's own deviation from float64 on that case;
positions relative to the cloud's extent, rotations by the angle between the two rotations (rad; q and -q are one rotation).  The
margin of 8 is the family's (tests/test_gpu_ik.py): another order of sums, and Horn's quaternion fit where the restatement uses an
SVD.  The reference's own recorded drags (tests/golden/arap_*.npz) hold for the kernel at tests/test_arap_cpu.py's bar plus that
parity bar.  The exact properties are bit equalities.  With RIGGS_ARAP_PARITY_JSON set to a path, what was measured is written there
under "gpu" (profiles/arap_parity.json is such a record).

Shapes (tests/arap_ref.py: CASES): N = 17 (K = 16 at its smallest N; fewer nodes than a wave), 65 (one node past a wave), 300 (not a
multiple of 64 nor of the 256 columns a wave reads per load; dropped edges present), 1024 (the limit); K in {4, 10, 16}; iterations
0, 1 and 3; ``init_verts`` given and not given; B in {1, 2, 3}."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from riggs_amd import arap as AR  # noqa: E402
from tests import arap_ref as R  # noqa: E402
from tests.pose_solve_util import T, bits  # noqa: E402
from tests.test_arap_cpu import BAR_POS, BAR_ROT  # noqa: E402

_REPORT, _GPU = {}, {}
BY_NAME = {c["name"]: c for c in R.CASES}
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arap_*.npz")))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    R.merge_report("RIGGS_ARAP_PARITY_JSON", "gpu", _REPORT)


def deformer(case):
    inp = R.case_inputs(case)
    return AR.ARAPDeformer(T(inp["verts"]), K=case["K"], radius=float(inp["radius"]), iterations=case["iterations"])


def case_gpu(case):
    """The kernel's result on a case (the whole batch in one launch): computed once, shared, never changed."""
    if case["name"] not in _GPU:
        inp, d = R.case_inputs(case), deformer(case)
        init = None if inp["init_verts"] is None else T(inp["init_verts"])
        pos, quat, none = d.deform_batch(list(inp["handles"]), T(inp["handle_pos"]), init_verts=init, return_R=True)
        assert none is None and pos.shape == (case["B"], case["N"], 3) and quat.shape == (case["B"], case["N"], 4)
        _GPU[case["name"]] = dict(d=d, pos=pos.cpu().numpy(), quat=quat.cpu().numpy(), nn_idx=d.nn_idx.cpu().numpy(),
                                  weight=d.weight.cpu().numpy())
    return _GPU[case["name"]]


@pytest.mark.parametrize("name", list(BY_NAME))
def test_parity_with_the_float64_oracle(name):
    case = BY_NAME[name]
    inp, got = R.case_inputs(case), case_gpu(case)
    # the graph, built by torch ops on the device, is the restatement's: it is the drag's input from here on
    r_idx, _, r_w = R.graph(inp["verts"], inp["radius"], case["K"])
    assert np.array_equal(got["nn_idx"], r_idx) and np.abs(got["weight"] - r_w).max() <= 1e-6
    if "blob" in name:
        assert (got["nn_idx"] < 0).any()
    o64, o32 = R.case_reference(case, got["nn_idx"], got["weight"])
    assert got["d"].null_dims == o64["null_dims"] == 0
    assert np.isfinite(got["pos"]).all() and np.isfinite(got["quat"]).all()
    ext = inp["extent"]
    dev = {"pos": float(np.abs(got["pos"] - o64["pos"]).max() / ext), "quat": float(R.rotation_angle(got["quat"], o64["quat"]).max())}
    e32 = {"pos": float(np.abs(o32["pos"] - o64["pos"]).max() / ext), "quat": float(R.rotation_angle(o32["quat"], o64["quat"]).max())}
    bar = {k: max(8 * e32[k], 1e-6) for k in e32}
    _REPORT[name] = {"e32": e32, "gpu": dev, "bar": bar}
    print(name, "e32", e32, "gpu", dev)
    failed = ["%s: %.3g > %.3g (e32 %.3g)" % (k, dev[k], bar[k], e32[k]) for k in dev if not dev[k] <= bar[k]]
    assert not failed, "; ".join(failed)
    # the handles sit on their targets bit for bit; the quaternions are unit (the identity for iterations = 0)
    assert np.array_equal(bits(got["pos"][:, list(inp["handles"])]), bits(inp["handle_pos"]))
    assert np.abs(np.linalg.norm(got["quat"].astype(np.float64), axis=-1) - 1).max() <= 1e-6
    if case["iterations"] == 0:
        assert np.array_equal(got["quat"], np.broadcast_to(np.float32([1, 0, 0, 0]), got["quat"].shape))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_the_references_recorded_drags(path):
    """ARAPDeformer / LapDeform as the reference is called, against what the reference returned: every recorded call, the chained
    ones from the reference's own previous positions.  Bar: the CPU test's (the float64 restatement against these goldens) plus
    this module's parity bar, max(8 * e32, 1e-6), with e32 measured on the golden's own calls."""
    with np.load(path) as z:
        g = {k: z[k] for k in z.files}
    ext = R.extent_of(g["verts"])
    if "trajectory" in g:
        tool = AR.LapDeform(T(g["verts"]), K=4, trajectory=T(g["trajectory"]), node_radius=torch.full((len(g["verts"]),), 0.1, device="cuda"))
        d, call = tool.arap_deformer, tool.deform_arap
        assert torch.equal(tool.init_pcl, T(g["verts"]))
    else:
        d = AR.ARAPDeformer(T(g["verts"]), K=int(g["K"]), radius=float(g["radius"]))
        call = d.deform
    assert d.K == int(g["K"]) and abs(float(d.radius) - float(g["radius"])) <= 1e-6 * float(g["radius"])
    assert np.array_equal(d.nn_idx.cpu().numpy(), g["nn"]) and np.abs(d.weight.cpu().numpy() - g["weight"]).max() <= 1e-6
    handles = tuple(int(v) for v in g["handle_idx"])
    G, _ = R.operator(R.laplacian(g["nn"], g["weight"]), handles)
    worst_p = worst_r = e32_p = e32_r = 0.0
    for c in range(len(g["pos"])):
        init = None if c == 0 else T(g["pos"][c - 1])
        # (handle_idx as a list, an array and a tensor; handle_pos as an array and a tensor)
        h = [g["handle_idx"].tolist(), g["handle_idx"], T(g["handle_idx"].astype(np.int64))][c % 3]
        hp = g["handle_pos"] if c % 2 == 0 else T(g["handle_pos"])
        pos, quat, none = call(h, hp, init_verts=init, return_R=True)
        assert none is None and pos.shape == g["pos"][c].shape and quat.shape == g["quat"][c].shape
        worst_p = max(worst_p, float(np.abs(pos.cpu().numpy() - g["pos"][c]).max() / ext))
        worst_r = max(worst_r, float(R.rotation_angle(quat.cpu().numpy(), g["quat"][c]).max()))
        assert torch.equal(call(h, hp, init_verts=init), pos)  # return_R=False: the positions alone
        host_init = None if c == 0 else g["pos"][c - 1]
        o64 = R.deform(g["verts"], g["nn"], g["weight"], G, handles, g["handle_pos"], host_init, 3, np.float64)
        o32 = R.deform(g["verts"], g["nn"], g["weight"], G.astype(np.float32), handles, g["handle_pos"], host_init, 3, np.float32)
        e32_p = max(e32_p, float(np.abs(o32[0] - o64[0]).max() / ext))
        e32_r = max(e32_r, float(R.rotation_angle(o32[1], o64[1]).max()))
    bar_p, bar_r = BAR_POS + max(8 * e32_p, 1e-6), BAR_ROT + max(8 * e32_r, 1e-6)
    _REPORT["golden-" + os.path.basename(path)[:-4]] = {"pos_over_extent": worst_p, "rot_rad": worst_r, "bar_pos": bar_p, "bar_rot": bar_r}
    print(os.path.basename(path), "positions %.3g of the extent, rotations %.3g rad" % (worst_p, worst_r))
    assert worst_p <= bar_p and worst_r <= bar_r, (worst_p, bar_p, worst_r, bar_r)


def test_a_drag_does_not_depend_on_its_batch_and_repeats_bit_for_bit():
    for name in ("n65_m3_b3_k16", "n65_m3_b3_k16_init"):
        case = BY_NAME[name]
        inp, got = R.case_inputs(case), case_gpu(case)
        d, h = got["d"], list(inp["handles"])
        init = None if inp["init_verts"] is None else T(inp["init_verts"][2])
        pos, quat, _ = d.deform(h, T(inp["handle_pos"][2]), init_verts=init, return_R=True)  # row 2 of the batch, alone
        assert np.array_equal(bits(pos.cpu().numpy()), bits(got["pos"][2])) and np.array_equal(bits(quat.cpu().numpy()), bits(got["quat"][2]))
        init = None if inp["init_verts"] is None else T(inp["init_verts"])
        again = d.deform_batch(h, T(inp["handle_pos"]), init_verts=init, return_R=True)
        assert np.array_equal(bits(again[0].cpu().numpy()), bits(got["pos"])) and np.array_equal(bits(again[1].cpu().numpy()), bits(got["quat"]))
    case = BY_NAME["n1024_m2_b2_k16"]
    inp, got = R.case_inputs(case), case_gpu(case)
    pos = got["d"].deform(list(inp["handles"]), T(inp["handle_pos"][1]))
    assert np.array_equal(bits(pos.cpu().numpy()), bits(got["pos"][1]))


def test_graph_capture_replays_with_new_targets():
    case = BY_NAME["n65_m3_b3_k16"]
    inp, got = R.case_inputs(case), case_gpu(case)
    d, h = got["d"], list(inp["handles"])
    hp = T(inp["handle_pos"][0]).clone()
    d.deform(h, hp, return_R=True)  # (the handle set's operator exists before the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d.deform(h, hp, return_R=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pos, quat, _ = d.deform(h, hp, return_R=True)
    hp.copy_(T(inp["handle_pos"][1]))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(pos.cpu().numpy()), bits(got["pos"][1])) and np.array_equal(bits(quat.cpu().numpy()), bits(got["quat"][1]))
    fresh = d.deform(h, T(inp["handle_pos"][1]), return_R=True)
    assert torch.equal(fresh[0], pos) and torch.equal(fresh[1], quat)


class _WavingNodes(torch.nn.Module):
    """A closed-form node network: every node sways with time."""

    def forward(self, x, t, **kwargs):
        z3, z4 = torch.zeros_like(x), torch.zeros(x.shape[0], 4, dtype=x.dtype, device=x.device)
        return {"d_xyz": 0.08 * torch.sin(6.283185307179586 * t + 3.0 * x), "d_rotation": z4, "d_scaling": z3,
                "local_rotation": z4.clone(), "hidden": None, "d_opacity": None, "d_color": None}


@pytest.mark.parametrize("use_traj", [True, False])
def test_animation_tool_drives_the_editing_path(use_traj):
    """animation_tool -> deform_arap -> forward(node_trans_bias=...) on a 2 000-Gaussian, 64-node warp."""
    from riggs_amd.control_nodes import ControlNodeWarp
    g = torch.Generator().manual_seed(21)
    x = (torch.rand(2000, 3, generator=g) - 0.5).cuda()
    cn = ControlNodeWarp(node_num=64, K=3, with_node_weight=True, local_frame=False, d_rot_as_res=True, hyper_dim=2, network=_WavingNodes()).cuda()
    with torch.no_grad():
        cn.nodes.copy_(torch.cat([x[torch.randperm(2000, generator=g)[:64].cuda()], torch.zeros(64, 2, device="cuda")], 1))
    t = torch.tensor(0.3, device="cuda")
    tool = cn.animation_tool(t, use_traj=use_traj)
    assert isinstance(tool, AR.LapDeform) and tool.init_pcl.shape == (64, 3) and tool.arap_deformer.K == 16
    handles = [5, 40]
    targets = (tool.init_pcl[handles] + torch.tensor([[0.2, 0.1, 0.0], [0.15, 0.12, -0.05]], device="cuda")).cpu().numpy()
    bias = tool.deform_arap(handles, targets, return_R=True)[0] - tool.init_pcl
    with torch.no_grad():
        out = cn(x, t, torch.zeros(2000, 2, device="cuda"), torch.ones(2000, 1, device="cuda"), node_trans_bias=bias)
    assert torch.isfinite(out["d_xyz"]).all() and float(out["d_xyz"].abs().max()) > 1e-2
    on = (out["d_nodes"].detach() + bias)[handles].cpu().numpy()
    assert np.abs(on - targets).max() <= 1e-6 * R.extent_of(tool.init_pcl.cpu().numpy())
    tool.reset()
    assert torch.equal(tool.init_pcl, tool.init_pcl_copy)


def test_argument_checks_raise_without_a_launch():
    v = torch.rand(30, 3, device="cuda")
    with pytest.raises(NotImplementedError):
        AR.ARAPDeformer(v, point_mask=torch.ones(30, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError):
        AR.ARAPDeformer(torch.rand(1025, 3, device="cuda"))
    with pytest.raises(ValueError):
        AR.ARAPDeformer(v, K=17)
    d = AR.ARAPDeformer(v, K=4, radius=10.0)
    for bad in ([], [30], [-1], [2, 2]):
        with pytest.raises(ValueError):
            d.deform(bad, np.zeros((len(bad), 3), np.float32))
    with pytest.raises(ValueError):
        d.deform([1, 2], np.zeros((3, 3), np.float32))  # (M targets for M handles)
    with pytest.raises(ValueError):
        d.deform([1], np.zeros((1, 3), np.float32), init_verts=torch.zeros(29, 3, device="cuda"))
    from riggs_amd import _lib as L
    with pytest.raises(L.RiggsHipError):  # (the C entry point's own checks: no launch either)
        L.check(L.lib().riggs_arap_edit(1, 1025, 4, 1, v.data_ptr(), 0, 0, 0, 1028, 0, 0, None, 3, 0, None, L.stream_ptr()), "riggs_arap_edit")
