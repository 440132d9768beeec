"""-m gpu: riggs_amd.pose_edit.solve_ik (csrc/ik.hip) against tests/ik_ref.py — float64 is the oracle, its float32 form the
yardstick for rounding.

Bars.  PARITY per case and tensor: max(8 * e32, 1e-6), e32 = the float32 restatement's own deviation from float64 on that case
(positions relative to the rig's extent); the margin of 8 because the kernel sums J J^T in another order and uses the
hardware's sin / cos / sqrt.  REACH: residual <= max(4 * r32, 1e-5 * extent) after 32 iterations, r32 the float32 restatement's
residual; the floor stands for a few float32 roundings through a chain of about 20 levels.  With RIGGS_IK_PARITY_JSON set to a
path, what was measured is written there (profiles/ik_parity.json is such a record)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import pose_edit as PE  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import ik_ref as R  # noqa: E402
from tests.pose_solve_util import T, bits, deviation, make_rig, parity_bars, parity_report  # noqa: E402

COUNTS = (8, 32)
KEYS = ("local_rotation", "global_trans", "d_nodes")
PARAMS = [(name, B) for name in R.CASES for B in (1, 3)]
IDS = ["%s-B%d" % p for p in PARAMS]
# What the solver's frame (csrc/pose_solve.h) does in each of its two forms (one wave: two_joints; 256 threads: tree65) and no case
# above asks of it (NOTES.md has the table): absolute damping and max_step (relative = 0: extent is NULL), one of the two (relative
# = 1, 2), the translation solved for beyond one joint, one handle on 256 threads.  3 problems, FEATURE_COUNTS iterations, the
# bars of the cases above.
FEATURES = {"absolute": dict(damping=0.07, max_step=0.6), "max_step": dict(max_step=0.6), "damping": dict(damping=0.07),
            "translation": dict(solve_translation=True), "one_handle": dict(E=1)}
FEATURE_COUNTS = (1, 4)
FEATURE_PARAMS = [(name, 3, f) for f in FEATURES for name in ("two_joints", "tree65") if (name, f) != ("two_joints", "one_handle")]
_CACHE, _REPORT = {}, {}
report = parity_report("RIGGS_IK_PARITY_JSON", _REPORT)


def run(case, iterations, **kw):
    """solve_ik on a case's batch -> numpy arrays (B, ...)."""
    pose = {"local_rotation": T(kw.pop("q0", case["q0"])), "global_trans": T(kw.pop("gt0", case["gt0"]))}
    handles = kw.pop("handles", case["handles"])
    targets = kw.pop("targets", case["targets"])
    for k in ("weights", "locked"):
        if kw.get(k) is not None:
            kw[k] = T(np.asarray(kw[k]))
    out = PE.solve_ik((T(case["joints"]), T(case["parents"])), pose, T(np.asarray(handles, np.int32)), T(targets), iterations=iterations,
                      solve_translation=case["solve_translation"], **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def feature_case(name, B, feature):
    """(the case with a FEATURES entry applied, what of the entry goes to the solver as keywords)."""
    case, kw = R.make_case(name, B), dict(FEATURES[feature] if feature else {})
    if kw.pop("E", None):
        case = dict(case, handles=case["handles"][:1], targets=np.ascontiguousarray(case["targets"][:, :1]), E=1)
    if kw.pop("solve_translation", False):
        case = dict(case, solve_translation=True)
    return case, kw


def reference(name, B, feature=None):
    """(case, float64 snapshots, float32 snapshots, GPU results) per iteration count: computed once, shared, never changed."""
    if (name, B, feature) not in _CACHE:
        case, kw = feature_case(name, B, feature)
        counts = FEATURE_COUNTS if feature else COUNTS
        o64 = R.solve_case(case, max(counts), np.float64, snapshots=counts, **kw)
        o32 = R.solve_case(case, max(counts), np.float32, snapshots=counts, **kw)
        gpu = {n: run(case, n, **kw) for n in counts}
        _CACHE[(name, B, feature)] = (case, o64, o32, gpu)
    return _CACHE[(name, B, feature)]


def bars(name, B, n, feature=None):
    """The parity bar of every tensor after n iterations, and e32 behind it."""
    case, o64, o32, _ = reference(name, B, feature)
    return parity_bars(o64[n], o32[n], KEYS, case["extent"])


@pytest.mark.parametrize("name,B,feature", [p + (None,) for p in PARAMS] + FEATURE_PARAMS, ids=IDS + ["%s-B%d-%s" % p for p in FEATURE_PARAMS])
def test_parity_with_the_float64_oracle(name, B, feature):
    case, o64, o32, gpu = reference(name, B, feature)
    failed = []
    for n in sorted(gpu):
        bar, e32 = bars(name, B, n, feature)
        dev = {k: deviation(gpu[n][k], o64[n][k], k, case["extent"]) for k in KEYS}
        _REPORT["%s-B%d-it%d" % ("-".join(filter(None, (name, feature))), B, n)] = {"e32": e32, "gpu": dev, "bar": bar,
                                               "residual_over_extent": {"float64": float(o64[n]["residual"].max() / case["extent"]),
                                                                        "float32": float(o32[n]["residual"].max() / case["extent"]),
                                                                        "gpu": float(gpu[n]["residual"].max() / case["extent"])}}
        print(name, B, feature, n, "e32", e32, "gpu", dev)
        failed += ["%s after %d iterations: %.3g > %.3g (e32 %.3g)" % (k, n, dev[k], bar[k], e32[k]) for k in KEYS if not dev[k] <= bar[k]]
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("name,B", PARAMS, ids=IDS)
def test_reach(name, B):
    case, o64, o32, gpu = reference(name, B)
    r32 = np.asarray(o32[32]["residual"], np.float64)
    got = np.asarray(gpu[32]["residual"], np.float64)
    print(name, B, "residual / extent: gpu", got.max() / case["extent"], "float32", r32.max() / case["extent"])
    assert np.isfinite(got).all() and (got <= np.maximum(4 * r32, 1e-5 * case["extent"])).all(), (got, r32)
    # residual is |target - posed handle| of the returned skeleton
    mine = np.sqrt(((case["targets"] - gpu[32]["d_nodes"][:, case["handles"]]) ** 2).sum(-1))
    assert np.abs(mine - got).max() <= 1e-6 * max(1.0, float(np.abs(case["targets"]).max()))


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_locked_and_off_path_joints_keep_their_bits(name):
    case = R.make_case(name, 3)
    on = R.paths(case["parents"], case["handles"])
    path = on.any(0)
    assert not path.all()  # (the case has joints that no handle's path visits)
    locked = np.zeros(case["J"], bool)
    locked[np.flatnonzero(path)[1::2]] = True  # every second joint of the paths
    out = run(case, 8, locked=locked)
    still = locked | ~path
    assert np.array_equal(bits(out["local_rotation"][:, still]), bits(case["q0"][:, still]))
    moved = out["local_rotation"][:, ~still] != case["q0"][:, ~still]
    assert moved.any(-1).all()  # ... and every other joint of the paths turned
    # a switched-off handle takes its path with it
    w = np.ones(case["E"], np.float32)
    w[0] = 0
    out = run(case, 8, weights=w)
    off = ~on[1:].any(0)
    assert on[0][off].any()
    assert np.array_equal(bits(out["local_rotation"][:, off]), bits(case["q0"][:, off]))


@pytest.mark.parametrize("name", ["root_only", "tree24", "tree256"])
def test_a_target_at_the_current_position_changes_nothing(name):
    case = R.make_case(name, 3)
    start = run(case, 0)  # no iteration: the forward kinematics of the starting pose
    assert np.array_equal(bits(start["local_rotation"]), bits(case["q0"])) and np.array_equal(bits(start["global_trans"]), bits(case["gt0"]))
    out = run(case, 8, targets=start["d_nodes"][:, case["handles"]])
    for k in KEYS:
        assert np.array_equal(bits(out[k]), bits(start[k])), k
    assert (out["residual"] == 0).all()


@pytest.mark.parametrize("name", ["tree24", "tree64", "tree256"])
def test_runs_are_bit_identical_and_problems_independent(name):
    case, _, _, gpu = reference(name, 3)
    again = run(case, 32)
    for k in KEYS + ("residual",):
        assert np.array_equal(bits(again[k]), bits(gpu[32][k])), k
    for b in range(case["B"]):
        one = dict(case, B=1, q0=case["q0"][b:b + 1], gt0=case["gt0"][b:b + 1], targets=case["targets"][b:b + 1])
        alone = run(one, 32)
        for k in KEYS + ("residual",):
            assert np.array_equal(bits(alone[k][0]), bits(gpu[32][k][b])), (k, b)


def test_weight_zero_is_the_problem_without_that_handle():
    name, B = "tree24", 3
    case = R.make_case(name, B)
    w = np.array([1, 0, 1], np.float32)
    with_zero = run(case, 32, weights=w)
    keep = [0, 2]
    without = dict(case, handles=case["handles"][keep], targets=np.ascontiguousarray(case["targets"][:, keep]), E=2)
    ref = run(without, 32)
    bar, _ = bars(name, B, 32)
    for k in KEYS:
        assert deviation(with_zero[k], ref[k], k, case["extent"]) <= bar[k], k
    assert np.abs(with_zero["residual"][:, keep] - ref["residual"]).max() / case["extent"] <= bar["d_nodes"]
    assert np.isfinite(with_zero["residual"]).all()  # (the switched-off handle's distance is still reported)
    # a negative and a NaN weight switch off as well
    for bad in (-1.0, float("nan")):
        w[1] = bad
        other = run(case, 32, weights=w)
        assert np.array_equal(bits(other["local_rotation"]), bits(with_zero["local_rotation"]))


def test_wave_form_and_workgroup_form_agree():
    name, B = "tree64", 3
    case, _, _, gpu = reference(name, B)
    joints = np.concatenate([case["joints"], 0.5 * (case["joints"][0:1] + case["joints"][1:2])]).astype(np.float32)  # (inside the box: same extent)
    assert R.extent_of(joints) == R.extent_of(case["joints"])
    parents = np.concatenate([case["parents"], [0]]).astype(np.int32)
    q0 = np.concatenate([case["q0"], np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1, 1))], 1)
    locked = np.zeros(65, bool)
    locked[64] = True
    wide = run(dict(case, joints=joints, parents=parents, q0=q0, J=65), 32, locked=locked)
    bar, _ = bars(name, B, 32)
    for k in KEYS:
        a = wide[k][:, :64] if k != "global_trans" else wide[k]
        assert deviation(a, gpu[32][k], k, case["extent"]) <= bar[k], k


def test_an_unreachable_target_stays_finite():
    """A target at 10 x extent.  Damped least squares with a damping far below the clamped step is not monotone on a stretched
    chain: the float64 restatement's residual swings by +-10 % between iteration 8 and 32 with the default damping of
    0.05 extent on every chain of three bones or more (chain4: 7.08, 6.98, 7.53, 7.29 at 8, 16, 24, 32), and falls monotonically
    once the damping is the clamped step, 0.5 extent (chain4: 6.9706, 6.9705, 6.9705, 6.9705; tree24: 12.80, 12.57, 12.51, 12.49;
    tree256: 28.21, 27.98, 27.84, 27.76).  So: finite with the default, and no growth from 8 to 32 at damping = max_step.
    Several handles pulled to ONE far point trade distance among themselves; what the iteration lowers is the norm of the
    whole residual vector of a problem (all weights are 1), so that is what must not grow — with one handle, the residual itself."""
    for name in ("chain4", "tree24", "tree256"):
        case = R.make_case(name, 3)
        ext = case["extent"]
        far = np.broadcast_to(case["joints"].mean(0) + np.float32(10 * ext) * np.array([0.6, 0.0, 0.8], np.float32), case["targets"].shape)
        far = np.ascontiguousarray(far, np.float32)
        loose = run(case, 32, targets=far)
        assert all(np.isfinite(loose[k]).all() for k in loose), name
        r8 = run(case, 8, targets=far, damping=0.5 * ext)
        r32 = run(case, 32, targets=far, damping=0.5 * ext)
        print(name, "residual at 8", r8["residual"].tolist(), "at 32", r32["residual"].tolist())
        assert all(np.isfinite(r32[k]).all() for k in r32), name
        norm = lambda r: np.sqrt((np.asarray(r, np.float64) ** 2).sum(-1))  # noqa: E731
        assert (norm(r32["residual"]) <= norm(r8["residual"])).all(), name


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_the_pose_goes_through_the_rig(name):
    from riggs_amd import synth
    from riggs_amd.viewer import skeleton_overlay
    case = R.make_case(name, 1)
    sw, x = make_rig(case)
    pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"])}
    out = PE.solve_ik(sw, pose, T(case["handles"]), T(case["targets"][0]), iterations=16)
    assert out["local_rotation"].shape == (case["J"], 4) and out["global_trans"].shape == (1, 3)
    assert out["d_nodes"].shape == (case["J"], 3) and out["residual"].shape == (case["E"],)
    d = sw.deform_by_pose(x, out, torch.ones(x.shape[0], 1, device="cuda"))
    U.assert_close(d["d_nodes"].detach().cpu().numpy(), out["d_nodes"].cpu().numpy(), "d_nodes of the IK pose through deform_by_pose", 1e-5)
    same = PE.solve_ik((T(case["joints"]), case["parents"]), pose, case["handles"].tolist(), T(case["targets"][0]), iterations=16)
    assert torch.equal(same["local_rotation"], out["local_rotation"])  # (host handles and parents: the same problem)
    table = skeleton_overlay(synth.look_at_camera(64, 64), out["d_nodes"], sw._parents_dev(x.device))
    assert tuple(table.shape) == (2 * case["J"] - 1, 12)


def test_capture_and_replay():
    case = R.make_case("tree24", 1)
    sw, x = make_rig(case)
    mask = torch.ones(x.shape[0], 1, device="cuda")
    q0, gt0 = T(case["q0"][0]), T(case["gt0"])
    handles, targets, weights = T(case["handles"]), T(case["targets"][0]), torch.ones(case["E"], device="cuda")

    @torch.no_grad()
    def step():
        out = PE.solve_ik(sw, {"local_rotation": q0, "global_trans": gt0}, handles, targets, weights=weights, iterations=16)
        return out, sw.deform_by_pose(x, out, mask)["d_xyz"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, d_xyz = step()
    g = torch.Generator().manual_seed(9)
    for rep in range(2):
        targets.add_(0.05 * torch.randn(targets.shape, generator=g).cuda())
        if rep == 1:
            weights[1] = 0.0
            handles[0] = case["handles"][1]
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_xyz = step()
        for k in eager:
            assert torch.equal(eager[k], out[k]), (rep, k)
        U.assert_close(d_xyz.cpu().numpy(), eager_xyz.cpu().numpy(), "d_xyz of the replay", 1e-6)


def test_refusals():
    case = R.make_case("tree24", 1)
    rig = (T(case["joints"]), T(case["parents"]))
    pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"])}
    tgt = T(case["targets"][0])
    with pytest.raises(L.RiggsHipError):  # E > 8
        PE.solve_ik(rig, pose, list(range(9)), torch.zeros(9, 3, device="cuda"))
    with pytest.raises(L.RiggsHipError):  # J > 256
        PE.solve_ik((torch.zeros(257, 3, device="cuda"), torch.zeros(257, dtype=torch.int32, device="cuda")),
                    {"local_rotation": torch.ones(257, 4, device="cuda"), "global_trans": torch.zeros(1, 3, device="cuda")}, [1], tgt[:1])
    for damping in (0.0, -0.1, float("nan")):
        with pytest.raises(L.RiggsHipError):
            PE.solve_ik(rig, pose, case["handles"].tolist(), tgt, damping=damping)
    for bad in (case["J"], -1):
        with pytest.raises(L.RiggsHipError):
            PE.solve_ik(rig, pose, [0, bad, 1], tgt)
    # the C entry refuses the same on its own: nothing is launched (the outputs keep their fill)
    out, buf = U.out_buf((case["J"], 4))
    z = torch.zeros(64, device="cuda")
    h = torch.zeros(16, dtype=torch.int32, device="cuda")
    for J, E, damping in ((case["J"], 9, 0.1), (257, 1, 0.1), (case["J"], 1, 0.0)):
        rc = L.lib().riggs_ik_solve(1, J, E, rig[0].data_ptr(), rig[1].data_ptr(), pose["local_rotation"].data_ptr(), z.data_ptr(),
                                    h.data_ptr(), z.data_ptr(), None, None, 4, damping, 1.0, None, 0, 0, out.data_ptr(), z.data_ptr(),
                                    z.data_ptr(), z.data_ptr(), L.stream_ptr())
        assert rc != 0
    torch.cuda.synchronize()
    assert bool((buf == U.SENT).all())
    # a handle index outside [0, J) that lives on the device is not read back: the kernel switches it off, its residual is NaN
    # (on one wave and on 256 threads)
    for case in (case, R.make_case("tree65", 1)):
        rig = (T(case["joints"]), T(case["parents"]))
        pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"])}
        tgt = T(case["targets"][0, :3])
        dev_handles = T(np.array([case["handles"][0], case["J"] + 5, case["handles"][2]], np.int32))
        got = PE.solve_ik(rig, pose, dev_handles, tgt, iterations=8)
        w = torch.tensor([1.0, 0.0, 1.0], device="cuda")
        ref = PE.solve_ik(rig, pose, T(case["handles"][:3]), tgt, weights=w, iterations=8)
        assert torch.equal(got["local_rotation"], ref["local_rotation"]) and bool(torch.isnan(got["residual"][1]))


def test_the_edit_step_on_the_device_is_the_one_on_the_host():
    """pick_joint -> joint_drag -> rotate_joint -> apply_edit with device tensors (the projection through viewer._project)
    against the same calls on CPU tensors, which tests/test_pose_edit_cpu.py holds to the reference's lines."""
    from riggs_amd import synth
    from riggs_amd.viewer import pick_joint
    cam = synth.look_at_camera(120, 160, azimuth_deg=30.0, elevation_deg=15.0, radius=3.0)
    case = R.make_case("tree8", 1)
    nodes, parents = torch.from_numpy(case["joints"]), torch.from_numpy(case["parents"]).long()
    uv = PE._project_editor(cam, nodes)
    pose = {"local_rotation": torch.from_numpy(case["q0"][0]), "global_trans": torch.from_numpy(case["gt0"])}
    for joint in (0, 3, 7):
        near = (float(uv[joint, 0]) + 0.4, float(uv[joint, 1]) + 0.4)
        idx = pick_joint(cam, nodes.cuda(), near)
        assert idx.is_cuda and int(idx) == joint
        mouse = (near[0] + 17.0, near[1] - 9.0)
        host = PE.joint_drag(cam, nodes, parents, joint, mouse, mouse_delta=(5.0, -3.0))
        dev = PE.joint_drag(cam, nodes.cuda(), parents.cuda(), idx, mouse, mouse_delta=(5.0, -3.0))
        assert dev[0].is_cuda and dev[1].is_cuda
        assert abs(float(dev[0]) - float(host[0])) <= 1e-5 and torch.equal(dev[1].cpu(), host[1])
        axis = PE.view_axis(cam)
        e_host = PE.rotate_joint(None, joint, axis, host[0], host[1], num_joints=8)
        e_dev = PE.rotate_joint(None, idx, axis.cuda(), dev[0], dev[1], num_joints=8)
        assert (e_dev["local_rotation"].cpu() - e_host["local_rotation"]).abs().max() <= 1e-5
        a_host = PE.apply_edit(pose, e_host)
        a_dev = PE.apply_edit({k: v.cuda() for k, v in pose.items()}, e_dev)
        assert (a_dev["local_rotation"].cpu() - a_host["local_rotation"]).abs().max() <= 1e-5
        assert (a_dev["global_trans"].cpu() - a_host["global_trans"]).abs().max() <= 1e-7
