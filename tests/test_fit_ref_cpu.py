"""tests/fit_ref.py (the NumPy restatement of riggs_amd.pose_edit.fit_pose, csrc/fit.hip) held to what it claims, without a GPU:
its two sweeps are the Jacobian of the tree and its transpose, one outer iteration solved to the end is one iteration of the IK
oracle (tests/ik_ref.py), the cases meet the conditions the GPU tests (tests/test_gpu_fit.py) rest on, and what ``fit_pose`` and
``riggs_fit_pose`` refuse before they touch a device."""
import ctypes

import numpy as np
import pytest
import torch

from riggs_amd import _abi
from riggs_amd import _lib as L
from riggs_amd import pose_edit as PE
from tests import fit_ref as F
from tests import ik_ref as R

KEYS = ("local_rotation", "global_trans", "d_nodes", "residual")
# what tests/fit_ref.py restates: where the function or its C entry is missing, this module has nothing to hold it to
FIT_POSE, FIT_ENTRY = PE.fit_pose, _abi.FUNCTIONS["riggs_fit_pose"]


def dense_jacobian(parents, posed, s, ext, locked):
    """(3J, 3J + 3): row block h, column block a = -s_h [posed_h - piv_a]x for the unlocked joints a on the path root .. h
    (tests/ik_ref.py: paths), and s_h extent I for tau'."""
    J = len(parents)
    vp = R.vparents(parents)
    on = R.paths(parents, np.arange(J))
    Jd = np.zeros((3 * J, 3 * J + 3))
    for h in range(J):
        for a in range(J):
            if on[h, a] and not locked[a]:
                Jd[3 * h:3 * h + 3, 3 * a:3 * a + 3] = -s[h] * R.cross_matrix(posed[h] - posed[vp[a]])
        Jd[3 * h:3 * h + 3, 3 * J:] = s[h] * ext * np.eye(3)
    return Jd


@pytest.mark.parametrize("name", ["two_joints", "chain4", "tree8", "tree24", "tree65"])
def test_the_sweeps_are_the_dense_jacobian_and_its_transpose(name):
    case = F.make_case(name, 1)
    J, parents = case["J"], case["parents"]
    rng = np.random.default_rng(3)
    posed = R.fk(case["joints"].astype(np.float64), parents, case["q0"][0].astype(np.float64), case["gt0"][0].astype(np.float64))[2]
    vp = R.vparents(parents)
    pc = posed - posed[0]
    pv = pc[vp]
    s = np.sqrt(rng.uniform(0.2, 2.0, J))
    s[rng.integers(0, J)] = 0.0  # (a joint without target)
    locked = np.zeros(J, bool)
    locked[1::3] = True
    ext = float(case["extent"])
    Jd = dense_jacobian(parents, posed, s, ext, locked)
    om, tau, u = rng.normal(0, 1, (J, 3)), rng.normal(0, 1, 3), rng.normal(0, 1, (J, 3))
    om[locked] = 0
    got = F.down(vp, pc, pv, s, om, ext * tau).reshape(-1)
    want = Jd @ np.concatenate([om.reshape(-1), tau])
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    g, gtau = F.up(vp, pc, pv, s, u, ~locked, ext)
    got = np.concatenate([g.reshape(-1), gtau])
    want = Jd.T @ u.reshape(-1)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the preconditioner's d_a from the moments about the posed root is the sum it stands for
    s2 = s * s
    S0, S1, S2 = F.subtree(vp, s2), F.subtree(vp, s2[:, None] * pc), F.subtree(vp, s2 * F.dot(pc, pc))
    dd = (S2 - 2 * F.dot(pv, S1)) + F.dot(pv, pv) * S0
    sub = R.paths(parents, np.arange(J)).T  # [a, h]: h in a's subtree
    want = np.array([(s2[sub[a]] * ((posed[sub[a]] - posed[vp[a]]) ** 2).sum(-1)).sum() for a in range(J)])
    assert np.abs(dd - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name,E", [("two_joints", 1), ("chain4", 2), ("tree8", 3), ("tree24", 8), ("tree65", 8)])
def test_one_iteration_solved_to_the_end_is_one_iteration_of_the_ik_oracle(name, E):
    """(J^T J + l^2 I)^-1 J^T = J^T (J J^T + l^2 I)^-1: the primal form with the CG run to the end (3J + 3 steps, no relative
    stop) against ik_ref.solve's dual form with the weighted joints as handles."""
    case = F.make_case(name, 1)
    J = case["J"]
    rng = np.random.default_rng(7)
    handles = np.sort(rng.choice(np.arange(1, J), size=min(E, J - 1), replace=False)).astype(np.int32)
    w_e = rng.uniform(0.5, 2.0, len(handles)).astype(np.float32)
    weights = np.zeros(J, np.float32)
    weights[handles] = w_e
    locked = np.zeros(J, bool)
    locked[2::5] = True
    fit = F.solve(case["joints"], case["parents"], case["q0"][0], case["gt0"][0], case["targets"][0], weights=weights, locked=locked,
                  iterations=1, cg_steps=3 * J + 3, cg_eps=0.0)
    ik = R.solve(case["joints"], case["parents"], case["q0"][0], case["gt0"][0], handles, case["targets"][0][handles], weights=w_e,
                 locked=locked, iterations=1)
    assert np.abs(fit["local_rotation"] - ik["local_rotation"]).max() <= 1e-9
    assert np.abs(fit["d_nodes"] - ik["d_nodes"]).max() <= 1e-9 * case["extent"]
    assert np.abs(fit["residual"][handles] - ik["residual"]).max() <= 1e-9 * case["extent"]
    assert (fit["residual"][weights <= 0] == 0).all()


def deviation(a, b, key, extent):
    d = float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    return d if key == "local_rotation" else d / extent


@pytest.mark.parametrize("name", F.PARITY)
def test_float32_stays_within_1e_4_of_float64_on_every_parity_case(name):
    for B in (1, 3):
        case, o64, o32 = F.reference(name, B)
        for n in F.SNAPSHOTS:
            e32 = {k: deviation(o32[n][k], o64[n][k], k, case["extent"]) for k in KEYS}
            print(name, B, n, e32)
            assert all(v <= 1e-4 for v in e32.values()), (name, B, n, e32)


@pytest.mark.parametrize("name", F.REACH)
def test_float64_reaches_the_targets_of_the_reach_cases(name):
    for B in (1, 3):
        case, o64, _ = F.reference(name, B)
        r = o64[32]["residual"].max() / case["extent"]
        print(name, B, "residual / extent", r)
        assert r <= 1e-4


@pytest.mark.parametrize("name", F.PARITY)
def test_the_early_stop_is_not_near_in_float64(name):
    """r.z / (r.z at the start) in front of every CG step is never within a factor of 100 of CG_EPS: the decision is not one that
    rounding could turn.  In every case but one the ratio stays above 1e-5 and no step is ever skipped.  two_joints is the
    exception, and it is decided as clearly the other way: both joints turn joint 1 about the same pivot, the right-hand side
    lies in ONE eigenspace of the preconditioned operator, the first CG step solves the system to rounding (ratio 1e-34 in
    float64, 1e-13 and less in float32) and the second step (cg_steps = min(8, J) = 2) is skipped in both precisions."""
    case = F.make_case(name, 3)
    for b in range(3):
        trace = []
        F.solve(case["joints"], case["parents"], case["q0"][b], case["gt0"][b], case["targets"][b], iterations=32,
                cg_steps=case["cg_steps"], solve_translation=case["solve_translation"], trace=trace)
        print(name, b, "smallest r.z ratio", min(trace) if trace else None)
        assert all(t >= 100 * F.CG_EPS or t <= F.CG_EPS / 100 for t in trace)
        assert name == "two_joints" or all(t >= 100 * F.CG_EPS for t in trace)
        if name == "two_joints":  # float32 decides as float64 does
            t32 = []
            F.solve(case["joints"], case["parents"], case["q0"][b], case["gt0"][b], case["targets"][b], iterations=32, cg_steps=2,
                    dtype=np.float32, trace=t32)
            print(name, b, "float32: largest ratio in front of a second step", max(t32[1::2]))
            assert all(t == 1.0 for t in t32[0::2]) and all(t <= F.CG_EPS / 100 for t in t32[1::2])


def test_a_nan_target_without_weight_is_never_used():
    case = F.make_case("tree8", 1)
    w = np.ones(8, np.float32)
    w[[3, 6]] = [0.0, -1.0]
    tg = case["targets"][0].copy()
    base = F.solve(case["joints"], case["parents"], case["q0"][0], case["gt0"][0], tg, weights=w, iterations=4, dtype=np.float32)
    tg[[3, 6]] = np.nan
    got = F.solve(case["joints"], case["parents"], case["q0"][0], case["gt0"][0], tg, weights=w, iterations=4, dtype=np.float32)
    for k in KEYS:
        assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), k


def test_refusals_that_need_no_device():
    case = F.make_case("tree8", 1)
    rig = (torch.from_numpy(case["joints"]), torch.from_numpy(case["parents"]))
    pose = {"local_rotation": torch.from_numpy(case["q0"][0]), "global_trans": torch.from_numpy(case["gt0"])}
    tg = torch.from_numpy(case["targets"][0])
    for steps in (0, -3):
        with pytest.raises(L.RiggsHipError, match="cg_steps"):
            PE.fit_pose(rig, pose, tg, cg_steps=steps)
    with pytest.raises(L.RiggsHipError, match="CUDA"):  # host tensors: no quiet CPU path
        PE.fit_pose(rig, pose, tg)
    # the binding is the header's, and the C entry refuses before it launches (the addresses are never read)
    assert len(_abi.FUNCTIONS["riggs_fit_pose"][1]) == 21
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(B=1, J=8, iterations=4, cg_steps=4, damping=0.1, max_step=1.0, extent=p, relative=0):
        return L.lib().riggs_fit_pose(B, J, p, p, p, p, p, None, None, iterations, cg_steps, damping, max_step, extent, relative, 0,
                                      p, p, p, p, None)
    for kw in (dict(B=0), dict(J=0), dict(J=257), dict(iterations=-1), dict(cg_steps=0), dict(damping=0.0), dict(damping=float("nan")),
               dict(max_step=-1.0), dict(extent=None), dict(relative=4)):
        assert call(**kw) != 0, kw
        assert "riggs_fit_pose" in L.lib().riggs_last_error().decode(), kw
