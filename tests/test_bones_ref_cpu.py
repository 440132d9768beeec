"""tests/bones_ref.py (the NumPy restatement of riggs_amd.pose_edit.fit_bones, csrc/bones.hip) held to what it claims, without a
GPU: its two sweeps are the Jacobian of the unit bone directions and its transpose, the cases meet the conditions the GPU tests
(tests/test_gpu_bones.py) rest on, ``bone_directions`` and ``retarget``'s root motion are their few-line restatements, and what
``fit_bones`` and ``riggs_fit_bones`` refuse before they touch a device."""
import ctypes

import numpy as np
import pytest
import torch

from riggs_amd import _abi
from riggs_amd import _lib as L
from riggs_amd import build as BUILD
from riggs_amd import pose_edit as PE
from tests import bones_ref as F
from tests import ik_ref as R

KEYS = ("local_rotation", "global_trans", "d_nodes", "residual")


def deviation(a, b, key, extent):
    """max |a - b|; positions and the translation relative to the rig's extent, the rest (rotations, chords) absolute."""
    d = float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    return d / extent if key in ("global_trans", "d_nodes") else d


def test_the_entry_is_declared_exported_and_built():
    assert len(_abi.FUNCTIONS["riggs_fit_bones"][1]) == 18
    assert hasattr(L.lib(), "riggs_fit_bones")
    assert _abi.CONSTANTS["RIGGS_ABI_VERSION"] == 102 and L.lib().riggs_version() == 102  # an added symbol: unchanged
    assert BUILD.SOURCES["bones.hip"] == ["-ffp-contract=off"]


@pytest.mark.parametrize("name", ["two_joints", "chain4", "tree8", "tree24", "tree65"])
def test_the_sweeps_are_the_jacobian_of_the_unit_directions_and_its_transpose(name):
    """Column block a of row block h is -s_h [d_h]x for the unlocked joints a on the path root .. h; and it IS the derivative:
    turning joint a by a small omega moves the posed unit directions by J omega (central differences on ik_ref.fk)."""
    case = F.make_case(name, 1)
    J, parents = case["J"], case["parents"]
    vp = R.vparents(parents)
    rng = np.random.default_rng(3)
    joints, q, gt = case["joints"].astype(np.float64), case["q0"][0].astype(np.float64), case["gt0"][0].astype(np.float64)

    def dirs(qq):
        posed = R.fk(joints, parents, qq, gt)[2]
        beta = posed - posed[vp]
        n = np.sqrt((beta ** 2).sum(-1))
        return np.where(n[:, None] > 0, beta / np.where(n > 0, n, 1)[:, None], 0)
    Rg = R.fk(joints, parents, q, gt)[0]
    d = dirs(q)
    s = np.sqrt(rng.uniform(0.2, 2.0, J))
    s[0] = 0.0
    s[rng.integers(1, J)] = 0.0  # (a bone without target)
    locked = np.zeros(J, bool)
    locked[1::3] = True
    on = R.paths(parents, np.arange(J))
    Jd = np.zeros((3 * J, 3 * J))
    for h in range(J):
        for a in range(J):
            if on[h, a] and not locked[a]:
                Jd[3 * h:3 * h + 3, 3 * a:3 * a + 3] = -s[h] * R.cross_matrix(d[h])
    om, u = rng.normal(0, 1, (J, 3)), rng.normal(0, 1, (J, 3))
    om[locked] = 0
    got, want = F.down(vp, d, s, om).reshape(-1), Jd @ om.reshape(-1)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    got, want = F.up(vp, d, s, u, ~locked).reshape(-1), Jd.T @ u.reshape(-1)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the derivative itself, one unlocked joint at a time
    eps = 1e-6
    for a in np.flatnonzero(~locked)[:4]:
        w = rng.normal(0, 1, 3)

        def turned(sign):
            delta = sign * eps * (w if a == 0 else Rg[vp[a]].T @ w)
            th = np.sqrt((delta ** 2).sum())
            qq = q.copy()
            qq[a] = R.quat_mul(np.concatenate([[np.cos(th / 2)], np.sin(th / 2) / th * delta]), q[a])
            return dirs(qq)
        numeric = s[:, None] * (turned(+1) - turned(-1)) / (2 * eps)
        e = np.zeros((J, 3))
        e[a] = w
        assert np.abs(numeric - F.down(vp, d, s, e)).max() <= 1e-8


@pytest.mark.parametrize("name", F.PARITY)
def test_float32_stays_within_1e_4_of_float64_on_every_parity_case(name):
    """The condition the GPU parity bars rest on: a condition on the inputs, not a measurement of the kernel."""
    for B in (1, 3):
        case, o64, o32 = F.reference(name, B)
        for n in F.SNAPSHOTS:
            e32 = {k: deviation(o32[n][k], o64[n][k], k, case["extent"]) for k in KEYS}
            print(name, B, n, e32)
            assert all(v <= 1e-4 for v in e32.values()), (name, B, n, e32)


@pytest.mark.parametrize("name", F.REACH)
def test_float64_reaches_the_directions_of_the_reach_cases(name):
    for B in (1, 3):
        case, o64, _ = F.reference(name, B)
        r = o64[32]["residual"].max()
        print(name, B, "largest chord", r)
        assert r <= 1e-5
        assert (o64[32]["residual"][:, 0] == 0).all()  # the root has no bone


def test_other_proportions_are_exercised_and_the_rig_keeps_its_own():
    case, o64, _ = F.reference("tree24", 3)
    vp = R.vparents(case["parents"])
    rest = np.sqrt(((case["joints"].astype(np.float64) - case["joints"][vp]) ** 2).sum(-1))
    src = np.sqrt((case["directions"].astype(np.float64) ** 2).sum(-1))
    ratio = src[:, 1:] / rest[1:]
    assert ratio.min() < 0.7 and ratio.max() > 1.5 and ratio.min() >= 0.5 - 1e-6 and ratio.max() <= 2 + 1e-6
    posed = o64[32]["d_nodes"]
    got = np.sqrt(((posed - posed[:, vp]) ** 2).sum(-1))
    assert np.abs(got - rest).max() <= 1e-12


def test_scaling_the_target_vectors_by_powers_of_two_changes_no_bit():
    case = F.make_case("tree8", 1)
    base = F.solve(case["joints"], case["parents"], case["q0"][0], case["gt0"][0], case["directions"][0], iterations=4, dtype=np.float32)
    scale = (2.0 ** np.random.default_rng(1).integers(-6, 7, (8, 1))).astype(np.float32)
    got = F.solve(case["joints"], case["parents"], case["q0"][0], case["gt0"][0], case["directions"][0] * scale, iterations=4, dtype=np.float32)
    for k in KEYS:
        assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), k


def test_a_target_that_is_off_is_never_used():
    """Weight 0, a negative weight, a zero-length rest bone and a zero target vector: the problem without that target."""
    case = F.make_case("tree8", 1)
    joints = case["joints"].copy()
    joints[5] = joints[case["parents"][5]]  # (joint 5 is a leaf of tree8)
    assert 5 not in case["parents"]
    w = np.ones(8, np.float32)
    w[[3, 6]] = [0.0, -1.0]
    tg = case["directions"][0].copy()
    tg[2] = 0
    w_off = w.copy()
    w_off[[2, 5]] = 0
    base = F.solve(joints, case["parents"], case["q0"][0], case["gt0"][0], case["directions"][0], weights=w_off, iterations=4, dtype=np.float32)
    got = F.solve(joints, case["parents"], case["q0"][0], case["gt0"][0], tg, weights=w, iterations=4, dtype=np.float32)
    tg[[3, 5, 6]] = np.nan
    nan = F.solve(joints, case["parents"], case["q0"][0], case["gt0"][0], tg, weights=w, iterations=4, dtype=np.float32)
    for k in KEYS:
        assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), k
        assert np.array_equal(nan[k].view(np.uint32), base[k].view(np.uint32)), k
    assert (base["residual"][[0, 2, 3, 5, 6]] == 0).all() and (base["residual"][[1, 4, 7]] > 0).all()


@pytest.mark.parametrize("name", F.PARITY)
def test_the_early_stop_is_not_near_in_float64(name):
    """r.z / (r.z at the start) in front of every CG step is never within a factor of 100 of CG_EPS: the decision to begin a
    step is not one that rounding could turn."""
    case = F.make_case(name, 3)
    for b in range(3):
        trace = []
        F.solve(case["joints"], case["parents"], case["q0"][b], case["gt0"][b], case["directions"][b], iterations=32,
                cg_steps=case["cg_steps"], trace=trace)
        print(name, b, "smallest r.z ratio", min(trace) if trace else None)
        assert all(t >= 100 * F.CG_EPS or t <= F.CG_EPS / 100 for t in trace)


def test_bone_directions_and_the_root_motion_match_their_restatements():
    rng = np.random.default_rng(5)
    joints, parents = R.tree(24, 15)
    J, Js, T = 24, 31, 5
    src = rng.normal(0, 1, (T, Js, 3)).astype(np.float32)
    jm = rng.permutation(Js)[:J].astype(np.int64)
    jm[[4, 17]] = -1
    for clip, m in ((src, jm), (src[0], jm), (src[:, :J], None)):
        want_d, want_w = F.bone_directions(clip, parents, m)
        got_d, got_w = PE.bone_directions(torch.from_numpy(clip), torch.from_numpy(parents), None if m is None else torch.from_numpy(m))
        assert got_d.shape == want_d.shape and got_w.shape == want_w.shape
        assert np.array_equal(got_d.numpy(), want_d) and np.array_equal(got_w.numpy(), want_w)
    want_d, want_w = F.bone_directions(src, parents, jm)
    vp = R.vparents(parents)
    off = np.zeros(J, bool)
    off[[4, 17]] = True
    off |= off[vp]  # a bone needs both ends
    off[0] = True
    assert (want_w[:, off] == 0).all() and (want_w[:, ~off] == 1).all() and (want_d[:, off] == 0).all() and off.sum() > 3
    with pytest.raises(L.RiggsHipError):  # Js != J without a map
        PE.bone_directions(torch.from_numpy(src), torch.from_numpy(parents))
    with pytest.raises(L.RiggsHipError):
        PE.bone_directions(torch.from_numpy(src), torch.from_numpy(parents), torch.from_numpy(jm[:-1]))
    # the root motion: k from the first frame's live bones, or given
    k = F.root_scale(joints, parents, src[0], jm)
    got = PE.root_follow(torch.from_numpy(joints), torch.from_numpy(parents), torch.from_numpy(src), torch.from_numpy(jm))
    want = F.root_follow(joints, src, jm, k)
    assert got.shape == (T, 3) and np.abs(got.numpy() - want).max() <= 1e-5 * np.abs(want).max()
    got = PE.root_follow(torch.from_numpy(joints), torch.from_numpy(parents), torch.from_numpy(src), torch.from_numpy(jm), root_scale=0.75)
    assert np.abs(got.numpy() - F.root_follow(joints, src, jm, 0.75)).max() <= 1e-6 * np.abs(want).max()
    jm0 = jm.copy()
    jm0[0] = -1  # the root is not mapped: the pose's translation stays
    keep = torch.tensor([[1.0, 2.0, 3.0]])
    got = PE.root_follow(torch.from_numpy(joints), torch.from_numpy(parents), torch.from_numpy(src), torch.from_numpy(jm0), global_trans=keep)
    assert torch.equal(got, keep.expand(T, 3))


def test_refusals_that_need_no_device():
    case = F.make_case("tree8", 1)
    rig = (torch.from_numpy(case["joints"]), torch.from_numpy(case["parents"]))
    pose = {"local_rotation": torch.from_numpy(case["q0"][0]), "global_trans": torch.from_numpy(case["gt0"])}
    tg = torch.from_numpy(case["directions"][0])
    for steps in (0, -3):
        with pytest.raises(L.RiggsHipError, match="cg_steps"):
            PE.fit_bones(rig, pose, tg, cg_steps=steps)
    with pytest.raises(L.RiggsHipError, match="CUDA"):  # host tensors: no quiet CPU path
        PE.fit_bones(rig, pose, tg)
    with pytest.raises(L.RiggsHipError, match="root_motion"):
        PE.retarget(rig, pose, tg, root_motion="sideways")
    # the C entry refuses before it launches (the addresses are never read)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(B=1, J=8, iterations=4, cg_steps=4, damping=0.1, max_step=1.0, directions=p, out=p):
        return L.lib().riggs_fit_bones(B, J, p, p, p, p, directions, None, None, iterations, cg_steps, damping, max_step, out, p, p, p, None)
    for kw in (dict(B=0), dict(J=0), dict(J=257), dict(iterations=-1), dict(cg_steps=0), dict(damping=0.0), dict(damping=float("nan")),
               dict(max_step=-1.0), dict(directions=None), dict(out=None)):
        assert call(**kw) != 0, kw
        assert "riggs_fit_bones" in L.lib().riggs_last_error().decode(), kw
