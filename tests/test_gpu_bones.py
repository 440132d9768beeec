"""-m gpu: riggs_amd.pose_edit.fit_bones / retarget (csrc/bones.hip) against tests/bones_ref.py — float64 is the oracle, its float32
form the yardstick for rounding.

Bars (those of tests/test_gpu_ik.py and tests/test_gpu_fit.py, for their reason).  PARITY per case, snapshot and tensor:
max(8 * e32, 1e-6), e32 = the float32 restatement's own deviation from float64 (positions and the translation relative to the rig's
extent; rotations and the residual, a chord of unit vectors, absolute); the margin of 8 stands for the hardware's sin / cos / sqrt
and whatever order of operations the restatement does not pin.  tests/test_bones_ref_cpu.py holds e32 <= 1e-4 on every case.
REACH: residual <= max(4 * r32, 1e-5) after 32 iterations, r32 the float32 restatement's residual.  With RIGGS_BONES_PARITY_JSON
set to a path, what was measured is written there (profiles/bones_parity.json is such a record)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import pose_edit as PE  # noqa: E402
from tests import bones_ref as F  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import ik_ref as R  # noqa: E402
from tests.pose_solve_util import T, bits, make_rig, parity_report  # noqa: E402

COUNTS = F.SNAPSHOTS
KEYS = ("local_rotation", "global_trans", "d_nodes", "residual")
PARAMS = [(name, B) for name in F.PARITY for B in (1, 3)]
_GPU, _REPORT = {}, {}
report = parity_report("RIGGS_BONES_PARITY_JSON", _REPORT)


def deviation(a, b, key, extent):
    d = float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    return d / extent if key in ("global_trans", "d_nodes") else d


def bars_of(o64, o32, extent):
    e32 = {k: deviation(o32[k], o64[k], k, extent) for k in KEYS}
    return {k: max(8 * e32[k], 1e-6) for k in KEYS}, e32


def run(case, iterations, **kw):
    """fit_bones on a case's batch -> numpy arrays (B, ...)."""
    pose = {"local_rotation": T(kw.pop("q0", case["q0"])), "global_trans": T(kw.pop("gt0", case["gt0"]))}
    directions = kw.pop("directions", case["directions"])
    joints = kw.pop("joints", case["joints"])
    for k in ("weights", "locked"):
        if kw.get(k) is not None:
            kw[k] = T(np.asarray(kw[k]))
    kw.setdefault("cg_steps", case["cg_steps"])
    out = PE.fit_bones((T(joints), T(case["parents"])), pose, T(directions), iterations=iterations, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def reference(name, B):
    """(case, float64 snapshots, float32 snapshots, GPU results) per iteration count: computed once, shared, never changed."""
    if (name, B) not in _GPU:
        case, o64, o32 = F.reference(name, B)
        _GPU[(name, B)] = (case, o64, o32, {n: run(case, n) for n in COUNTS})
    return _GPU[(name, B)]


def unit_bones(d_nodes, parents):
    vp = R.vparents(parents)
    beta = np.asarray(d_nodes, np.float64)
    beta = beta - beta[..., vp, :]
    n = np.sqrt((beta ** 2).sum(-1))
    return beta / np.where(n > 0, n, 1)[..., None], n


def unit(v):
    v = np.asarray(v, np.float64)
    n = np.sqrt((v ** 2).sum(-1))
    return v / np.where(n > 0, n, 1)[..., None]


@pytest.mark.parametrize("name,B", PARAMS, ids=["%s-B%d" % p for p in PARAMS])
def test_parity_with_the_float64_oracle(name, B):
    case, o64, o32, gpu = reference(name, B)
    failed = []
    for n in sorted(gpu):
        bar, e32 = bars_of(o64[n], o32[n], case["extent"])
        dev = {k: deviation(gpu[n][k], o64[n][k], k, case["extent"]) for k in KEYS}
        _REPORT["%s-B%d-it%d" % (name, B, n)] = {"e32": e32, "gpu": dev, "bar": bar,
                                                 "gpu_over_e32": {k: (dev[k] / e32[k] if e32[k] > 0 else None) for k in KEYS},
                                                 "largest_chord": {"float64": float(o64[n]["residual"].max()),
                                                                   "float32": float(o32[n]["residual"].max()),
                                                                   "gpu": float(gpu[n]["residual"].max())}}
        print(name, B, n, "e32", e32, "gpu", dev)
        failed += ["%s after %d iterations: %.3g > %.3g (e32 %.3g)" % (k, n, dev[k], bar[k], e32[k]) for k in KEYS if not dev[k] <= bar[k]]
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("name,B", [(name, B) for name in F.REACH for B in (1, 3)])
def test_reach(name, B):
    case, o64, o32, gpu = reference(name, B)
    r32 = np.asarray(o32[32]["residual"], np.float64)
    got = np.asarray(gpu[32]["residual"], np.float64)
    print(name, B, "largest chord: gpu", got.max(), "float32", r32.max())
    assert np.isfinite(got).all() and (got <= np.maximum(4 * r32, 1e-5)).all(), (got, r32)
    # residual is the chord |t - d| of the returned skeleton's bones
    d, _ = unit_bones(gpu[32]["d_nodes"], case["parents"])
    mine = np.sqrt(((unit(case["directions"]) - d) ** 2).sum(-1))
    mine[:, 0] = 0
    assert np.abs(mine - got).max() <= 2e-6  # (float32 positions of up to an extent, subtracted and normalised: a few 1e-7)


@pytest.mark.parametrize("name", ["tree24", "tree64"])
def test_other_proportions_are_met_and_the_rig_keeps_its_own(name):
    """The source's bones are 0.5 to 2 times the rig's: the returned skeleton points along them and has the RIG's rest lengths."""
    case, _, o32, gpu = reference(name, 3)
    vp = R.vparents(case["parents"])
    rest = np.sqrt(((case["joints"].astype(np.float64) - case["joints"][vp]) ** 2).sum(-1))
    src = np.sqrt((case["directions"].astype(np.float64) ** 2).sum(-1))
    assert (src[:, 1:] / rest[1:]).min() < 0.7 and (src[:, 1:] / rest[1:]).max() > 1.5
    d, length = unit_bones(gpu[32]["d_nodes"], case["parents"])
    chord = np.sqrt(((unit(case["directions"]) - d) ** 2).sum(-1))[:, 1:]
    print(name, "largest chord from d_nodes", chord.max(), "largest |length - rest| / extent", np.abs(length - rest).max() / case["extent"])
    assert (chord <= np.maximum(4 * np.asarray(o32[32]["residual"], np.float64)[:, 1:], 1e-5) + 2e-6).all()
    assert np.abs(length - rest).max() <= 1e-5 * case["extent"]


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_scaling_the_target_vectors_changes_no_bit(name):
    case, _, _, gpu = reference(name, 3)
    by4 = run(case, 32, directions=case["directions"] * np.float32(4.0))
    scale = (2.0 ** np.random.default_rng(1).integers(-6, 7, (1, case["J"], 1))).astype(np.float32)
    bonewise = run(case, 32, directions=case["directions"] * scale)
    for k in KEYS:
        assert np.array_equal(bits(by4[k]), bits(gpu[32][k])), k
        assert np.array_equal(bits(bonewise[k]), bits(gpu[32][k])), k


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_a_target_that_is_off_is_the_problem_without_it(name):
    """Weight 0, a zero-length rest bone (a leaf put on its parent) and a zero target vector give, bit for bit, the problem in which
    those weights are 0, and residual 0 there; a NaN in such a row changes no bit (rows without weight or rest length are never
    read, and a NaN vector fails |v| > 0).  The kernel agrees with the oracle of THAT problem within its parity bar."""
    B, n = 3, 8
    case = F.make_case(name, B)
    J = case["J"]
    leaves = [i for i in range(1, J) if i not in set(case["parents"].tolist())]
    zero_rest, zero_vec, no_weight = leaves[0], leaves[1], [3, leaves[2]]
    joints = case["joints"].copy()
    joints[zero_rest] = joints[case["parents"][zero_rest]]
    w = np.ones((B, J), np.float32)
    w[:, no_weight] = 0
    w[1, 5] = 0  # (per problem)
    tg = case["directions"].copy()
    tg[:, zero_vec] = 0
    w_off = w.copy()
    w_off[:, [zero_rest, zero_vec]] = 0
    moved = dict(case, joints=joints)
    base = run(moved, n, joints=joints, weights=w_off)
    got = run(moved, n, joints=joints, directions=tg, weights=w)
    o64 = F.solve_case(moved, n, np.float64, weights=w_off)
    o32 = F.solve_case(moved, n, np.float32, weights=w_off)
    bar, e32 = bars_of(o64, o32, case["extent"])
    for k in KEYS:
        assert np.array_equal(bits(got[k]), bits(base[k])), k
        print(k, "e32", e32[k], "gpu", deviation(base[k], o64[k], k, case["extent"]))
        assert deviation(base[k], o64[k], k, case["extent"]) <= bar[k], k
    assert (got["residual"][w_off <= 0] == 0).all() and (got["residual"][:, 0] == 0).all() and np.isfinite(got["residual"]).all()
    junk = tg.copy()
    junk[w <= 0] = np.nan
    junk[:, [0, zero_rest, zero_vec]] = np.nan
    other = run(moved, n, joints=joints, directions=junk, weights=w)
    for k in KEYS:
        assert np.isfinite(other[k]).all() and np.array_equal(bits(other[k]), bits(base[k])), k
    for bad in (-1.0, float("nan")):  # a negative and a NaN weight switch off as well
        w2 = w.copy()
        w2[w <= 0] = bad
        other = run(moved, n, joints=joints, directions=tg, weights=w2)
        assert np.array_equal(bits(other["local_rotation"]), bits(base["local_rotation"]))


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_locked_joints_and_joints_without_a_live_bone_below_them_keep_their_bits(name):
    case = F.make_case(name, 3)
    J = case["J"]
    below = R.paths(case["parents"], np.arange(J)).T  # [a, h]: h is in a's subtree
    a = max(range(1, J), key=lambda i: (min(int(below[i].sum()), 6), -i))  # a joint with a few joints below it
    assert below[a].sum() >= 2
    w = np.ones(J, np.float32)
    w[below[a]] = 0  # no live bone in a's subtree (a's own bone included): nothing there is observed
    locked = np.zeros(J, bool)
    locked[np.flatnonzero(~below[a])[1::2]] = True
    out = run(case, 8, weights=w, locked=locked)
    still = locked | below[a]
    assert np.array_equal(bits(out["local_rotation"][:, still]), bits(case["q0"][:, still]))
    free = np.flatnonzero(~still)
    has_bone_below = np.array([(below[i] & (w > 0) & (np.arange(J) != 0)).any() for i in free])
    moved = (out["local_rotation"][:, free] != case["q0"][:, free]).any(-1)
    assert moved[:, has_bone_below].all()  # ... and every other joint with a bone to turn turned
    assert (out["residual"][:, below[a]] == 0).all() and np.isfinite(out["residual"]).all()
    assert np.array_equal(bits(out["global_trans"]), bits(case["gt0"]))


@pytest.mark.parametrize("name", ["two_joints", "tree24", "tree256"])
def test_directions_already_met_change_nothing(name):
    """Start = the second pose, on the unscaled rig; the targets are the bones of its posed skeleton as the kernel's own forward
    kinematics gives them (a run of 0 iterations), scaled bone-wise by powers of two: t = d bit for bit, every step is zero, and
    the unobserved twist stays where it was."""
    case = F.make_case(name, 3)
    start = run(case, 0, q0=case["q1"])
    assert np.array_equal(bits(start["local_rotation"]), bits(case["q1"])) and np.array_equal(bits(start["global_trans"]), bits(case["gt0"]))
    vp = R.vparents(case["parents"])
    scale = (2.0 ** np.random.default_rng(2).integers(-1, 2, (1, case["J"], 1))).astype(np.float32)
    out = run(case, 8, q0=case["q1"], directions=(start["d_nodes"] - start["d_nodes"][:, vp]) * scale)
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
        one = dict(case, B=1, q0=case["q0"][b:b + 1], gt0=case["gt0"][b:b + 1], directions=case["directions"][b:b + 1])
        alone = run(one, 32)
        for k in KEYS:
            assert np.array_equal(bits(alone[k][0]), bits(gpu[32][k][b])), (k, b)


def test_wave_form_and_workgroup_form_give_the_same_bits():
    """tree64 with one more leaf without weight (J = 65: 256 threads, the sweeps through LDS) against the 64-joint problem on one
    wave: BIT-IDENTICAL.  The order of every sum is the same — the new leaf is the root's last child and hands it zeros first,
    the first wave's tree over its 64 joints is the wave form's, and the other three waves add zeros."""
    name, B = "tree64", 3
    case, _, _, gpu = reference(name, B)
    joints = np.concatenate([case["joints"], 0.5 * (case["joints"][0:1] + case["joints"][1:2])]).astype(np.float32)
    parents = np.concatenate([case["parents"], [0]]).astype(np.int32)
    q0 = np.concatenate([case["q0"], np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1, 1))], 1)
    directions = np.concatenate([case["directions"], np.full((B, 1, 3), np.nan, np.float32)], 1)
    w = np.ones(65, np.float32)
    w[64] = 0
    wide = run(dict(case, parents=parents, J=65), 32, joints=joints, q0=q0, directions=directions, weights=w)
    for k in KEYS:
        a = wide[k][:, :64] if k != "global_trans" else wide[k]
        assert np.array_equal(bits(a), bits(gpu[32][k])), k
    assert np.array_equal(bits(wide["local_rotation"][:, 64]), bits(q0[:, 64])) and (wide["residual"][:, 64] == 0).all()


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_the_pose_goes_through_the_rig(name):
    case = F.make_case(name, 3)
    sw, x = make_rig(case)
    mask = torch.ones(x.shape[0], 1, device="cuda")
    pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"][0:1])}
    out = PE.fit_bones(sw, pose, T(case["directions"][0]), iterations=8)
    assert out["local_rotation"].shape == (case["J"], 4) and out["global_trans"].shape == (1, 3)
    assert out["d_nodes"].shape == (case["J"], 3) and out["residual"].shape == (case["J"],)
    assert torch.equal(out["global_trans"], pose["global_trans"])
    d = sw.deform_by_pose(x, out, mask)
    U.assert_close(d["d_nodes"].detach().cpu().numpy(), out["d_nodes"].cpu().numpy(), "d_nodes of the fitted pose through deform_by_pose", 1e-5)
    same = PE.fit_bones((T(case["joints"]), case["parents"]), pose, T(case["directions"][0]), iterations=8)
    assert torch.equal(same["local_rotation"], out["local_rotation"])  # (host parents: the same problem)
    track = PE.fit_bones(sw, {"local_rotation": T(case["q0"]), "global_trans": T(case["gt0"])}, T(case["directions"]), iterations=8)
    assert track["local_rotation"].shape == (3, case["J"], 4) and track["global_trans"].shape == (3, 3)
    assert torch.equal(track["local_rotation"][0], out["local_rotation"])
    seq = sw.deform_sequence(x, track, mask)
    U.assert_close(seq["d_nodes"].cpu().numpy(), track["d_nodes"].cpu().numpy(), "d_nodes of the fitted track through deform_sequence", 1e-5)


def test_capture_and_replay():
    case = F.make_case("tree24", 1)
    sw, x = make_rig(case)
    mask = torch.ones(x.shape[0], 1, device="cuda")
    q0, gt0 = T(case["q0"][0]), T(case["gt0"])
    directions, weights = T(case["directions"][0]), torch.ones(case["J"], device="cuda")

    @torch.no_grad()
    def step():
        out = PE.fit_bones(sw, {"local_rotation": q0, "global_trans": gt0}, directions, weights=weights, iterations=8)
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
        directions.add_(0.05 * torch.randn(directions.shape, generator=g).cuda())
        if rep == 1:
            weights[5] = 0.0
            directions[5] = float("nan")
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_xyz = step()
        for k in eager:
            assert torch.equal(eager[k], out[k]), (rep, k)
        U.assert_close(d_xyz.cpu().numpy(), eager_xyz.cpu().numpy(), "d_xyz of the replay", 1e-6)


def test_retarget_a_clip_with_two_joints_dropped():
    """T = 5 frames of a source skeleton with more joints, other proportions and its own joint order, two rig joints unmapped:
    frame by frame the restatement's problem (bones_ref.bone_directions, root_follow, solve), within the parity bar."""
    name, frames, n = "tree24", 5, 8
    case = F.make_case(name, frames)
    J, parents, joints = case["J"], case["parents"], case["joints"]
    rng = np.random.default_rng(77)
    Js = J + 4
    jm = rng.permutation(Js)[:J].astype(np.int64)
    src = rng.normal(0, 1, (frames, Js, 3)).astype(np.float32)
    other = F.rescaled(joints, parents, rng.uniform(0.5, 2.0, J))  # one performer: the same proportions in every frame
    for t in range(frames):  # the mapped joints: the second pose on the rescaled copy of the rig, walking along x
        src[t, jm] = R.fk(other, parents, case["q1"][t].astype(np.float64), np.array([0.1 * t, 0.0, 0.0]))[2]
    dropped = [6, 19]
    jm[dropped] = -1
    dirs, w = F.bone_directions(src, parents, jm)
    k = F.root_scale(joints, parents, src[0], jm)
    gt = F.root_follow(joints, src, jm, k).astype(np.float32)
    sw, x = make_rig(case)
    pose = {"local_rotation": T(case["q0"]), "global_trans": T(case["gt0"][0:1])}
    out = PE.retarget(sw, pose, T(src), joint_map=T(jm), root_motion="follow", iterations=n)
    got = {k_: v.cpu().numpy() for k_, v in out.items()}
    assert got["local_rotation"].shape == (frames, J, 4) and got["global_trans"].shape == (frames, 3) and got["d_nodes"].shape == (frames, J, 3)
    assert np.abs(got["global_trans"] - gt).max() <= 1e-5 * max(1.0, np.abs(gt).max())
    want = dict(case, gt0=got["global_trans"])  # (the translation as the device formed it: the solve is what is compared)
    o64 = F.solve_case(want, n, np.float64, directions=dirs, weights=w)
    o32 = F.solve_case(want, n, np.float32, directions=dirs, weights=w)
    bar, e32 = bars_of(o64, o32, case["extent"])
    for key in KEYS:
        print(key, "e32", e32[key], "gpu", deviation(got[key], o64[key], key, case["extent"]))
        assert deviation(got[key], o64[key], key, case["extent"]) <= bar[key], key
    off = (w <= 0)
    assert off[:, dropped].all() and (got["residual"][off] == 0).all()
    # the same frames as fit_bones takes them, and the track through the rig
    same = PE.fit_bones(sw, {"local_rotation": T(case["q0"]), "global_trans": out["global_trans"]}, T(dirs), weights=T(w), iterations=n)
    assert torch.equal(same["local_rotation"], out["local_rotation"])
    mask = torch.ones(x.shape[0], 1, device="cuda")
    seq = sw.deform_sequence(x, out, mask)
    U.assert_close(seq["d_nodes"].cpu().numpy(), got["d_nodes"], "d_nodes of the retargeted track through deform_sequence", 1e-5)
    fixed = PE.retarget(sw, pose, T(src), joint_map=T(jm), root_motion="follow", root_scale=0.5, iterations=0)
    assert np.abs(fixed["global_trans"].cpu().numpy() - F.root_follow(joints, src, jm, 0.5)).max() <= 1e-5 * max(1.0, np.abs(gt).max())
    none = PE.retarget(sw, pose, T(src), joint_map=T(jm), iterations=0)
    assert torch.equal(none["global_trans"], pose["global_trans"].expand(frames, 3))


def test_refusals():
    case = F.make_case("tree24", 3)
    J = case["J"]
    rig = (T(case["joints"]), T(case["parents"]))
    pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"][0:1])}
    tgt = T(case["directions"][0])
    with pytest.raises(L.RiggsHipError):  # J = 0
        PE.fit_bones((torch.zeros(0, 3, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")),
                     {"local_rotation": torch.ones(0, 4, device="cuda"), "global_trans": torch.zeros(1, 3, device="cuda")},
                     torch.zeros(0, 3, device="cuda"))
    with pytest.raises(L.RiggsHipError):  # J > 256
        PE.fit_bones((torch.zeros(257, 3, device="cuda"), torch.zeros(257, dtype=torch.int32, device="cuda")),
                     {"local_rotation": torch.ones(257, 4, device="cuda"), "global_trans": torch.zeros(1, 3, device="cuda")},
                     torch.zeros(257, 3, device="cuda"))
    for steps in (0, -1):
        with pytest.raises(L.RiggsHipError):
            PE.fit_bones(rig, pose, tgt, cg_steps=steps)
    for damping in (0.0, -0.1, float("nan")):
        with pytest.raises(L.RiggsHipError):
            PE.fit_bones(rig, pose, tgt, damping=damping)
    with pytest.raises(L.RiggsHipError):
        PE.fit_bones(rig, pose, tgt, max_step=-1.0)
    with pytest.raises(L.RiggsHipError):
        PE.fit_bones(rig, pose, tgt, iterations=-1)
    for bad in (tgt[:-1], tgt[:, :2], tgt.reshape(-1), tgt[None, None]):  # wrong shapes
        with pytest.raises(L.RiggsHipError):
            PE.fit_bones(rig, pose, bad)
    with pytest.raises(L.RiggsHipError):
        PE.fit_bones(rig, pose, tgt, weights=torch.ones(J - 1, device="cuda"))
    with pytest.raises(L.RiggsHipError):
        PE.fit_bones(rig, pose, tgt, locked=torch.zeros(J + 1, dtype=torch.bool))
    with pytest.raises(L.RiggsHipError):  # mismatched batch sizes
        PE.fit_bones(rig, {"local_rotation": T(case["q0"]), "global_trans": T(case["gt0"])}, T(case["directions"][:2]))
    with pytest.raises(L.RiggsHipError):  # no quiet CPU path
        PE.fit_bones(rig, pose, tgt.cpu())
    with pytest.raises(L.RiggsHipError):  # J + 1 source joints and no map
        PE.retarget(rig, pose, torch.zeros(2, J + 1, 3, device="cuda"))
    with pytest.raises(L.RiggsHipError):
        PE.retarget(rig, pose, torch.zeros(2, J, 3, device="cuda"), root_motion="sideways")
    # the C entry refuses the same on its own: nothing is launched (the outputs keep their fill)
    out, buf = U.out_buf((J, 4))
    z = torch.zeros(4 * 257, device="cuda")
    for Jc, steps, damping, dirs in ((0, 4, 0.1, z), (257, 4, 0.1, z), (J, 0, 0.1, z), (J, 4, 0.0, z), (J, 4, 0.1, None)):
        rc = L.lib().riggs_fit_bones(1, Jc, rig[0].data_ptr(), rig[1].data_ptr(), pose["local_rotation"].data_ptr(), z.data_ptr(),
                                     L.ptr(dirs), None, None, 4, steps, damping, 1.0, out.data_ptr(), z.data_ptr(), z.data_ptr(),
                                     z.data_ptr(), L.stream_ptr())
        assert rc != 0
    torch.cuda.synchronize()
    assert bool((buf == U.SENT).all())
