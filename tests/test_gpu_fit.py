"""-m gpu: riggs_amd.pose_edit.fit_pose (csrc/fit.hip) against tests/fit_ref.py — float64 is the oracle, its float32 form the
yardstick for rounding.

Bars (those of tests/test_gpu_ik.py, for its reason).  PARITY per case, snapshot and tensor: max(8 * e32, 1e-6), e32 = the
float32 restatement's own deviation from float64 (positions, the translation and the residual relative to the rig's extent); the
margin of 8 stands for the hardware's sin / cos / sqrt and whatever order of operations the restatement does not pin.
tests/test_fit_ref_cpu.py holds e32 <= 1e-4 on every case.  REACH: residual <= max(4 * r32, 1e-5 * extent) after 32 iterations,
r32 the float32 restatement's residual.  With RIGGS_FIT_PARITY_JSON set to a path, what was measured is written there
(profiles/fit_parity.json is such a record)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import pose_edit as PE  # noqa: E402
from tests import fit_ref as F  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import ik_ref as R  # noqa: E402
from tests.pose_solve_util import T, bits, deviation, make_rig, parity_bars, parity_report  # noqa: E402

COUNTS = F.SNAPSHOTS
KEYS = ("local_rotation", "global_trans", "d_nodes", "residual")
PARAMS = [(name, B) for name in F.PARITY for B in (1, 3)]
IDS = ["%s-B%d" % p for p in PARAMS]
# What the solver's frame (csrc/pose_solve.h) does in each of its two forms (one wave: two_joints; 256 threads: tree65) and no case
# above asks of it (NOTES.md has the table): absolute damping and max_step (relative = 0), one of the two (relative = 1, 2), the
# translation solved for beyond one joint; and of the solver's own, one CG step on 256 threads and more CG steps than joints.
# 3 problems, FEATURE_COUNTS iterations, the bars of the cases above.
FEATURES = {"absolute": dict(damping=0.07, max_step=0.6), "max_step": dict(max_step=0.6), "damping": dict(damping=0.07),
            "translation": dict(solve_translation=True), "one_cg_step": dict(cg_steps=1), "cg_steps_over_J": dict(cg_steps=8)}
FEATURE_COUNTS = (1, 4)
FEATURE_PARAMS = [(name, 3, f) for f in FEATURES for name in ("two_joints", "tree65")
                  if (name, f) not in (("two_joints", "one_cg_step"), ("tree65", "cg_steps_over_J"))]
_GPU, _REPORT = {}, {}
report = parity_report("RIGGS_FIT_PARITY_JSON", _REPORT)


def run(case, iterations, **kw):
    """fit_pose on a case's batch -> numpy arrays (B, ...)."""
    pose = {"local_rotation": T(kw.pop("q0", case["q0"])), "global_trans": T(kw.pop("gt0", case["gt0"]))}
    targets = kw.pop("targets", case["targets"])
    for k in ("weights", "locked"):
        if kw.get(k) is not None:
            kw[k] = T(np.asarray(kw[k]))
    kw.setdefault("cg_steps", case["cg_steps"])
    kw.setdefault("solve_translation", case["solve_translation"])
    out = PE.fit_pose((T(case["joints"]), T(case["parents"])), pose, T(targets), iterations=iterations, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def reference(name, B, feature=None):
    """(case, float64 snapshots, float32 snapshots, GPU results) per iteration count: computed once, shared, never changed."""
    if (name, B, feature) not in _GPU:
        if feature is None:
            case, o64, o32 = F.reference(name, B)
            kw, counts = {}, COUNTS
        else:
            case, kw, counts = F.make_case(name, B), FEATURES[feature], FEATURE_COUNTS
            o64 = F.solve_case(case, max(counts), np.float64, snapshots=counts, **kw)
            o32 = F.solve_case(case, max(counts), np.float32, snapshots=counts, **kw)
        _GPU[(name, B, feature)] = (case, o64, o32, {n: run(case, n, **kw) for n in counts})
    return _GPU[(name, B, feature)]


def bars_of(o64, o32, extent):
    return parity_bars(o64, o32, KEYS, extent)


@pytest.mark.parametrize("name,B,feature", [p + (None,) for p in PARAMS] + FEATURE_PARAMS, ids=IDS + ["%s-B%d-%s" % p for p in FEATURE_PARAMS])
def test_parity_with_the_float64_oracle(name, B, feature):
    case, o64, o32, gpu = reference(name, B, feature)
    failed = []
    for n in sorted(gpu):
        bar, e32 = bars_of(o64[n], o32[n], case["extent"])
        dev = {k: deviation(gpu[n][k], o64[n][k], k, case["extent"]) for k in KEYS}
        _REPORT["%s-B%d-it%d" % ("-".join(filter(None, (name, feature))), B, n)] = {"e32": e32, "gpu": dev, "bar": bar,
                                               "gpu_over_e32": {k: (dev[k] / e32[k] if e32[k] > 0 else None) for k in KEYS},
                                               "residual_over_extent": {"float64": float(o64[n]["residual"].max() / case["extent"]),
                                                                        "float32": float(o32[n]["residual"].max() / case["extent"]),
                                                                        "gpu": float(gpu[n]["residual"].max() / case["extent"])}}
        print(name, B, feature, n, "e32", e32, "gpu", dev)
        failed += ["%s after %d iterations: %.3g > %.3g (e32 %.3g)" % (k, n, dev[k], bar[k], e32[k]) for k in KEYS if not dev[k] <= bar[k]]
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("name,B", [(name, B) for name in F.REACH for B in (1, 3)])
def test_reach(name, B):
    case, o64, o32, gpu = reference(name, B)
    r32 = np.asarray(o32[32]["residual"], np.float64)
    got = np.asarray(gpu[32]["residual"], np.float64)
    print(name, B, "residual / extent: gpu", got.max() / case["extent"], "float32", r32.max() / case["extent"])
    assert np.isfinite(got).all() and (got <= np.maximum(4 * r32, 1e-5 * case["extent"])).all(), (got, r32)
    # residual is |target - posed joint| of the returned skeleton
    mine = np.sqrt(((case["targets"] - gpu[32]["d_nodes"]) ** 2).sum(-1))
    assert np.abs(mine - got).max() <= 1e-6 * max(1.0, float(np.abs(case["targets"]).max()))


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_locked_joints_and_joints_without_a_target_below_them_keep_their_bits(name):
    case = F.make_case(name, 3)
    J = case["J"]
    below = R.paths(case["parents"], np.arange(J)).T  # [a, h]: h is in a's subtree
    a = max(range(1, J), key=lambda i: (min(int(below[i].sum()), 6), -i))  # a joint with a few joints below it
    assert below[a].sum() >= 2
    w = np.ones(J, np.float32)
    w[below[a]] = 0  # no target in a's subtree: nothing below a is observed
    locked = np.zeros(J, bool)
    locked[np.flatnonzero(~below[a])[1::2]] = True
    out = run(case, 8, weights=w, locked=locked)
    still = locked | below[a]
    assert np.array_equal(bits(out["local_rotation"][:, still]), bits(case["q0"][:, still]))
    moved = out["local_rotation"][:, ~still] != case["q0"][:, ~still]
    free = np.flatnonzero(~still)
    has_target_below = np.array([(below[i] & (w > 0) & (np.arange(J) != 0)).any() for i in free])
    assert moved.any(-1)[:, has_target_below].all()  # ... and every other joint with a target to reach turned
    assert (out["residual"][:, below[a]] == 0).all() and np.isfinite(out["residual"]).all()


@pytest.mark.parametrize("name", ["root_only", "tree24", "tree256"])
def test_targets_at_the_current_posed_joints_change_nothing(name):
    case = F.make_case(name, 3)
    start = run(case, 0)  # no iteration: the forward kinematics of the starting pose
    assert np.array_equal(bits(start["local_rotation"]), bits(case["q0"])) and np.array_equal(bits(start["global_trans"]), bits(case["gt0"]))
    out = run(case, 8, targets=start["d_nodes"])
    for k in ("local_rotation", "global_trans", "d_nodes"):
        assert np.array_equal(bits(out[k]), bits(start[k])), k
    assert (out["residual"] == 0).all()


@pytest.mark.parametrize("name", ["tree24", "tree64", "tree256"])
def test_runs_are_bit_identical_and_problems_independent(name):
    case, _, _, gpu = reference(name, 3)
    again = run(case, 32)
    for k in KEYS:
        assert np.array_equal(bits(again[k]), bits(gpu[32][k])), k
    for b in range(case["B"]):
        one = dict(case, B=1, q0=case["q0"][b:b + 1], gt0=case["gt0"][b:b + 1], targets=case["targets"][b:b + 1])
        alone = run(one, 32)
        for k in KEYS:
            assert np.array_equal(bits(alone[k][0]), bits(gpu[32][k][b])), (k, b)


def test_weight_zero_is_the_problem_without_that_target():
    """The oracle leaves a joint without weight out of every sum; the kernel agrees with it within the parity bar of THIS
    problem, whatever stands in the unweighted targets (which it never reads): a NaN, an infinity and 1e30 give the same bits."""
    name, B, n = "tree24", 3, 8
    case = F.make_case(name, B)
    w = np.ones((B, case["J"]), np.float32)
    w[:, [3, 10, 23]] = 0
    w[1, 5] = 0  # (per problem)
    o64 = F.solve_case(case, n, np.float64, weights=w)
    o32 = F.solve_case(case, n, np.float32, weights=w)
    got = run(case, n, weights=w)
    bar, e32 = bars_of(o64, o32, case["extent"])
    for k in KEYS:
        print(k, "e32", e32[k], "gpu", deviation(got[k], o64[k], k, case["extent"]))
        assert deviation(got[k], o64[k], k, case["extent"]) <= bar[k], k
    assert (got["residual"][w <= 0] == 0).all()
    for junk in (np.nan, np.inf, 1e30):
        tg = case["targets"].copy()
        tg[w <= 0] = junk
        other = run(case, n, targets=tg, weights=w)
        for k in KEYS:
            assert np.isfinite(other[k]).all() and np.array_equal(bits(other[k]), bits(got[k])), (junk, k)
    for bad in (-1.0, float("nan")):  # a negative and a NaN weight switch off as well
        w2 = w.copy()
        w2[w <= 0] = bad
        other = run(case, n, weights=w2)
        assert np.array_equal(bits(other["local_rotation"]), bits(got["local_rotation"]))


def test_wave_form_and_workgroup_form_give_the_same_bits():
    """tree64 with one more leaf without weight (J = 65: 256 threads, the sweeps through LDS) against the 64-joint problem on one
    wave: BIT-IDENTICAL.  The order of every sum is the same — the new leaf is the root's last child and hands it zeros first,
    the first wave's tree over its 64 joints is the wave form's, and the other three waves add zeros."""
    name, B = "tree64", 3
    case, _, _, gpu = reference(name, B)
    joints = np.concatenate([case["joints"], 0.5 * (case["joints"][0:1] + case["joints"][1:2])]).astype(np.float32)  # (inside the box: same extent)
    assert R.extent_of(joints) == R.extent_of(case["joints"])
    parents = np.concatenate([case["parents"], [0]]).astype(np.int32)
    q0 = np.concatenate([case["q0"], np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1, 1))], 1)
    targets = np.concatenate([case["targets"], np.full((B, 1, 3), np.nan, np.float32)], 1)
    w = np.ones(65, np.float32)
    w[64] = 0
    wide = run(dict(case, joints=joints, parents=parents, q0=q0, J=65), 32, targets=targets, weights=w)
    for k in KEYS:
        a = wide[k][:, :64] if k != "global_trans" else wide[k]
        assert np.array_equal(bits(a), bits(gpu[32][k])), k
    assert np.array_equal(bits(wide["local_rotation"][:, 64]), bits(q0[:, 64])) and (wide["residual"][:, 64] == 0).all()


def test_unreachable_targets_stay_finite_and_translation_brings_them_back():
    for name in ("chain4", "tree8", "tree256"):
        case = F.make_case(name, 3)
        far = (case["targets"] + np.float32(10 * case["extent"]) * np.array([0.6, 0.0, 0.8], np.float32)).astype(np.float32)
        for n in (8, 32):
            out = run(case, n, targets=far)
            assert all(np.isfinite(out[k]).all() for k in out), (name, n)
    case = F.make_case("tree8", 3)
    ext = case["extent"]
    far = (case["targets"] + np.float32(10 * ext) * np.array([0.6, 0.0, 0.8], np.float32)).astype(np.float32)
    r32 = np.asarray(F.solve_case(case, 32, np.float32, targets=far, solve_translation=True)["residual"], np.float64)
    got = np.asarray(run(case, 32, targets=far, solve_translation=True)["residual"], np.float64)
    print("tree8 shifted by 10 extents, solve_translation: residual / extent gpu", got.max() / ext, "float32", r32.max() / ext)
    assert np.isfinite(got).all() and (got <= np.maximum(4 * r32, 1e-5 * ext)).all(), (got, r32)


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_the_pose_goes_through_the_rig(name):
    case = F.make_case(name, 3)
    sw, x = make_rig(case)
    mask = torch.ones(x.shape[0], 1, device="cuda")
    pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"][0:1])}
    out = PE.fit_pose(sw, pose, T(case["targets"][0]), iterations=8)
    assert out["local_rotation"].shape == (case["J"], 4) and out["global_trans"].shape == (1, 3)
    assert out["d_nodes"].shape == (case["J"], 3) and out["residual"].shape == (case["J"],)
    d = sw.deform_by_pose(x, out, mask)
    U.assert_close(d["d_nodes"].detach().cpu().numpy(), out["d_nodes"].cpu().numpy(), "d_nodes of the fitted pose through deform_by_pose", 1e-5)
    same = PE.fit_pose((T(case["joints"]), case["parents"]), pose, T(case["targets"][0]), iterations=8)
    assert torch.equal(same["local_rotation"], out["local_rotation"])  # (host parents: the same problem)
    # a clip of joint positions -> a pose track: the (B, J, 4) result feeds deform_sequence unchanged
    track = PE.fit_pose(sw, {"local_rotation": T(case["q0"]), "global_trans": T(case["gt0"])}, T(case["targets"]), iterations=8)
    assert track["local_rotation"].shape == (3, case["J"], 4) and track["global_trans"].shape == (3, 3)
    assert torch.equal(track["local_rotation"][0], out["local_rotation"])
    seq = sw.deform_sequence(x, track, mask)
    U.assert_close(seq["d_nodes"].cpu().numpy(), track["d_nodes"].cpu().numpy(), "d_nodes of the fitted track through deform_sequence", 1e-5)


def test_capture_and_replay():
    case = F.make_case("tree24", 1)
    sw, x = make_rig(case)
    mask = torch.ones(x.shape[0], 1, device="cuda")
    q0, gt0 = T(case["q0"][0]), T(case["gt0"])
    targets, weights = T(case["targets"][0]), torch.ones(case["J"], device="cuda")

    @torch.no_grad()
    def step():
        out = PE.fit_pose(sw, {"local_rotation": q0, "global_trans": gt0}, targets, weights=weights, iterations=8)
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
            weights[5] = 0.0
            targets[5] = float("nan")
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_xyz = step()
        for k in eager:
            assert torch.equal(eager[k], out[k]), (rep, k)
        U.assert_close(d_xyz.cpu().numpy(), eager_xyz.cpu().numpy(), "d_xyz of the replay", 1e-6)


def test_refusals():
    case = F.make_case("tree24", 3)
    J = case["J"]
    rig = (T(case["joints"]), T(case["parents"]))
    pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"][0:1])}
    tgt = T(case["targets"][0])
    with pytest.raises(L.RiggsHipError):  # J = 0
        PE.fit_pose((torch.zeros(0, 3, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")),
                    {"local_rotation": torch.ones(0, 4, device="cuda"), "global_trans": torch.zeros(1, 3, device="cuda")},
                    torch.zeros(0, 3, device="cuda"))
    with pytest.raises(L.RiggsHipError):  # J > 256
        PE.fit_pose((torch.zeros(257, 3, device="cuda"), torch.zeros(257, dtype=torch.int32, device="cuda")),
                    {"local_rotation": torch.ones(257, 4, device="cuda"), "global_trans": torch.zeros(1, 3, device="cuda")},
                    torch.zeros(257, 3, device="cuda"))
    for steps in (0, -1):
        with pytest.raises(L.RiggsHipError):
            PE.fit_pose(rig, pose, tgt, cg_steps=steps)
    for damping in (0.0, -0.1, float("nan")):
        with pytest.raises(L.RiggsHipError):
            PE.fit_pose(rig, pose, tgt, damping=damping)
    with pytest.raises(L.RiggsHipError):
        PE.fit_pose(rig, pose, tgt, max_step=-1.0)
    with pytest.raises(L.RiggsHipError):
        PE.fit_pose(rig, pose, tgt, iterations=-1)
    for bad in (tgt[:-1], tgt[:, :2], tgt.reshape(-1), tgt[None, None]):  # wrong shapes
        with pytest.raises(L.RiggsHipError):
            PE.fit_pose(rig, pose, bad)
    with pytest.raises(L.RiggsHipError):
        PE.fit_pose(rig, pose, tgt, weights=torch.ones(J - 1, device="cuda"))
    with pytest.raises(L.RiggsHipError):
        PE.fit_pose(rig, pose, tgt, locked=torch.zeros(J + 1, dtype=torch.bool))
    with pytest.raises(L.RiggsHipError):
        PE.fit_pose(rig, {"local_rotation": T(case["q0"][0][:, :3]), "global_trans": pose["global_trans"]}, tgt)
    with pytest.raises(L.RiggsHipError):  # mismatched batch sizes
        PE.fit_pose(rig, {"local_rotation": T(case["q0"]), "global_trans": T(case["gt0"])}, T(case["targets"][:2]))
    with pytest.raises(L.RiggsHipError):
        PE.fit_pose(rig, pose, T(case["targets"]), weights=torch.ones(2, J, device="cuda"))
    with pytest.raises(L.RiggsHipError):  # no quiet CPU path
        PE.fit_pose(rig, pose, tgt.cpu())
    # the C entry refuses the same on its own: nothing is launched (the outputs keep their fill)
    out, buf = U.out_buf((J, 4))
    z = torch.zeros(4 * 257, device="cuda")
    ext = torch.ones(1, device="cuda")
    for Jc, steps, damping, e in ((0, 4, 0.1, ext), (257, 4, 0.1, ext), (J, 0, 0.1, ext), (J, 4, 0.0, ext), (J, 4, 0.1, None)):
        rc = L.lib().riggs_fit_pose(1, Jc, rig[0].data_ptr(), rig[1].data_ptr(), pose["local_rotation"].data_ptr(), z.data_ptr(),
                                    z.data_ptr(), None, None, 4, steps, damping, 1.0, L.ptr(e), 0, 0, out.data_ptr(), z.data_ptr(),
                                    z.data_ptr(), z.data_ptr(), L.stream_ptr())
        assert rc != 0
    torch.cuda.synchronize()
    assert bool((buf == U.SENT).all())
