"""tests/rays_ref.py (the NumPy restatement of riggs_amd.pose_edit.fit_rays, csrc/rays.hip) held to what it claims, without a GPU: its
operator is the dense J^T diag(N) J and its sweeps are the halves, pins alone are tests/fit_ref.py's problem and three orthogonal
rays are a pin of twice their weight, the cases meet the conditions the GPU tests (tests/test_gpu_rays.py) rest on, ``camera_rays``
inverts csrc/pinhole.h's rule, and what ``fit_rays`` and ``riggs_fit_rays`` refuse before they touch a device."""
import ctypes

import numpy as np
import pytest
import torch

from riggs_amd import _abi
from riggs_amd import _lib as L
from riggs_amd import pose_edit as PE
from riggs_amd import synth
from riggs_amd.loss import camera_intrinsics
from tests import fit_ref as F
from tests import ik_ref as R
from tests import rays_ref as Y

KEYS = ("local_rotation", "global_trans", "d_nodes", "residual")
# what tests/rays_ref.py restates: where the function or its C entry is missing, this module has nothing to hold it to
FIT_RAYS, RAYS_ENTRY = PE.fit_rays, _abi.FUNCTIONS["riggs_fit_rays"]


def dense_jacobian(parents, posed, ext, locked):
    """(3J, 3J + 3): row block h, column block a = -[posed_h - piv_a]x for the unlocked joints a on the path root .. h, and
    extent I for tau' (tests/test_fit_ref_cpu.py's, without the weights: they are the metric's here)."""
    J = len(parents)
    vp = R.vparents(parents)
    on = R.paths(parents, np.arange(J))
    Jd = np.zeros((3 * J, 3 * J + 3))
    for h in range(J):
        for a in range(J):
            if on[h, a] and not locked[a]:
                Jd[3 * h:3 * h + 3, 3 * a:3 * a + 3] = -R.cross_matrix(posed[h] - posed[vp[a]])
        Jd[3 * h:3 * h + 3, 3 * J:] = ext * np.eye(3)
    return Jd


def full_metric(N):
    J = len(N)
    D = np.zeros((3 * J, 3 * J))
    for h in range(J):
        xx, yy, zz, xy, xz, yz = N[h]
        D[3 * h:3 * h + 3, 3 * h:3 * h + 3] = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
    return D


@pytest.mark.parametrize("name", ["two_joints", "chain4", "tree8", "tree24", "tree65"])
def test_the_operator_is_the_dense_one_and_the_sweeps_are_its_halves(name):
    case = Y.make_case(name, 1, 3, "mixed" if name in ("tree24", "tree65") else "rays")
    J, parents = case["J"], case["parents"]
    rng = np.random.default_rng(3)
    posed = R.fk(case["joints"].astype(np.float64), parents, case["q0"][0].astype(np.float64), case["gt0"][0].astype(np.float64))[2]
    vp = R.vparents(parents)
    pc = posed - posed[0]
    pv = pc[vp]
    weights = rng.uniform(0.2, 2.0, (J, 3)).astype(np.float32) if case["weights"] is None else case["weights"][0]
    pins = None if case["pins"] is None else case["pins"][0]
    w, o, d, wp, t, N, n = Y.constraints(case["origins"][0], case["directions"][0], weights, pins,
                                         None if pins is None else case["pin_weights"][0], J, np.float64)
    D = full_metric(N)
    for h in range(J):  # N_h is what it stands for
        want = wp[h] * np.eye(3) + sum(w[h, k] * (np.eye(3) - np.outer(d[h, k], d[h, k])) for k in range(3))
        assert np.abs(D[3 * h:3 * h + 3, 3 * h:3 * h + 3] - want).max() <= 1e-12
        assert abs(n[h] - np.trace(want) / 3) <= 1e-12
    locked = np.zeros(J, bool)
    locked[1::3] = True
    ext = float(case["extent"])
    Jd = dense_jacobian(parents, posed, ext, locked)
    om, tau, u = rng.normal(0, 1, (J, 3)), rng.normal(0, 1, 3), rng.normal(0, 1, (J, 3))
    om[locked] = 0
    x = np.concatenate([om.reshape(-1), tau])
    got = Y.down(vp, pc, pv, om, ext * tau).reshape(-1)
    want = Jd @ x
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    g, gtau = Y.up(vp, pc, pv, u, ~locked, ext)
    got = np.concatenate([g.reshape(-1), gtau])
    want = Jd.T @ u.reshape(-1)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    g, gtau = Y.up(vp, pc, pv, Y.metric(N, Y.down(vp, pc, pv, om, ext * tau)), ~locked, ext)
    got = np.concatenate([g.reshape(-1), gtau])
    want = Jd.T @ (D @ (Jd @ x))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the preconditioner's d_a from the moments of n about the posed root is the sum it stands for
    S0, S1, S2 = F.subtree(vp, n), F.subtree(vp, n[:, None] * pc), F.subtree(vp, n * F.dot(pc, pc))
    dd = (S2 - 2 * F.dot(pv, S1)) + F.dot(pv, pv) * S0
    sub = R.paths(parents, np.arange(J)).T  # [a, h]: h in a's subtree
    want = np.array([(n[sub[a]] * ((posed[sub[a]] - posed[vp[a]]) ** 2).sum(-1)).sum() for a in range(J)])
    assert np.abs(dd - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", ["tree8", "tree24"])
def test_pins_alone_are_fit_pose(name):
    case = F.make_case(name, 1)
    J = case["J"]
    w = np.random.default_rng(5).uniform(0.5, 2.0, J).astype(np.float32)
    w[[2, J - 1]] = [0.0, -1.0]
    args = (case["joints"], case["parents"], case["q0"][0], case["gt0"][0])
    want = F.solve(*args, case["targets"][0], weights=w, iterations=8, cg_steps=case["cg_steps"])
    got = Y.solve(*args, pins=case["targets"][0], pin_weights=w, iterations=8, cg_steps=case["cg_steps"])
    for k in KEYS:
        assert np.abs(got[k] - want[k]).max() <= 1e-9, k


@pytest.mark.parametrize("name", ["tree8", "tree24"])
def test_three_orthogonal_rays_through_a_point_are_a_pin_of_twice_the_weight(name):
    """sum over an orthonormal triple of w (I - d d^T) = 2 w I, and the three clamped errors sum to 2 w (target - posed) where
    max_step is out of the way.  The rays are float64 (a float32 direction is orthogonal to 1e-7 only)."""
    case = F.make_case(name, 1)
    J = case["J"]
    rng = np.random.default_rng(6)
    w = rng.uniform(0.5, 2.0, J).astype(np.float32)
    targets = case["targets"][0].astype(np.float64)
    basis = np.stack([np.linalg.qr(rng.normal(0, 1, (3, 3)))[0].T for _ in range(J)])            # (J, 3, 3): rows orthonormal
    directions = basis * rng.uniform(0.5, 3.0, (J, 3, 1))                                        # (any length)
    origins = targets[:, None, :] + rng.normal(0, 2.0, (J, 3, 1)) * basis                        # somewhere on each line
    args = (case["joints"], case["parents"], case["q0"][0], case["gt0"][0])
    want = F.solve(*args, case["targets"][0], weights=2 * w, iterations=8, cg_steps=case["cg_steps"], max_step=1e6)
    got = Y.solve(*args, origins=origins, directions=directions, weights=np.repeat(w[:, None], 3, 1), iterations=8,
                  cg_steps=case["cg_steps"], max_step=1e6)
    for k in ("local_rotation", "global_trans", "d_nodes"):
        assert np.abs(got[k] - want[k]).max() <= 1e-9, k
    # (the residual is the largest distance to one of the three lines: at most the distance to the point)
    assert (got["residual"] <= want["residual"] + 1e-9).all()


def deviation(a, b, key, extent):
    d = float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    return d if key == "local_rotation" else d / extent


@pytest.mark.parametrize("name,K,kind", Y.PARITY, ids=["%s-K%d-%s" % p for p in Y.PARITY])
def test_float32_stays_within_1e_4_of_float64_on_every_parity_case(name, K, kind):
    for B in (1, 3):
        case, o64, o32 = Y.reference(name, B, K, kind)
        for n in Y.snapshots_of(name, K, kind):
            e32 = {k: deviation(o32[n][k], o64[n][k], k, case["extent"]) for k in KEYS}
            print(name, K, kind, B, n, e32)
            assert all(v <= 1e-4 for v in e32.values()), (name, K, kind, B, n, e32)


@pytest.mark.parametrize("name,K,kind", Y.PARITY, ids=["%s-K%d-%s" % p for p in Y.PARITY])
def test_the_yardstick_is_stable_under_a_start_one_ulp_away(name, K, kind):
    """e32 is ONE draw of the rounding.  A second draw — the float32 restatement started one ulp away — stays within
    STABLE * max(e32, 1.25e-7) of float64, half of what the GPU bar allows the kernel (tests/rays_ref.py: STABLE)."""
    for B in (1, 3):
        case, o64, o32 = Y.reference(name, B, K, kind)
        moved = Y.moved_start(name, B, K, kind)
        for n in Y.snapshots_of(name, K, kind):
            e32 = {k: deviation(o32[n][k], o64[n][k], k, case["extent"]) for k in KEYS}
            m32 = {k: deviation(moved[n][k], o64[n][k], k, case["extent"]) for k in KEYS}
            print(name, K, kind, B, n, "moved / e32", {k: m32[k] / max(e32[k], 1.25e-7) for k in KEYS})
            assert all(m32[k] <= Y.STABLE * max(e32[k], 1.25e-7) for k in KEYS), (name, K, kind, B, n, e32, m32)


def test_a_dropped_snapshot_is_the_last_one_of_a_large_tree():
    assert all(R.CASES[name][0] >= 64 for name, _, _ in Y.DROP_32) and set(Y.DROP_32) <= set(Y.PARITY)


@pytest.mark.parametrize("name,K", Y.REACH)
def test_float64_reaches_the_rays_of_the_reach_cases(name, K):
    for B in (1, 3):
        case, o64, _ = Y.reference(name, B, K)
        r = o64[32]["residual"].max() / case["extent"]
        print(name, K, B, "residual / extent", r)
        assert r <= 1e-4


@pytest.mark.parametrize("name,K,kind", Y.PARITY, ids=["%s-K%d-%s" % p for p in Y.PARITY])
def test_the_early_stop_is_not_near_in_float64(name, K, kind):
    """r.z / (r.z at the start) in front of every CG step of the float64 references is never within a factor of 100 of CG_EPS:
    the decision is not one that rounding could turn.  Where a step is skipped at all, it is decided as clearly the other way."""
    for B in (1, 3):
        Y.reference(name, B, K, kind)
        trace = Y.TRACES[(name, B, K, kind)]
        small = [t for t in trace if t < 100 * F.CG_EPS]
        print(name, K, kind, B, "smallest r.z ratio", min(trace) if trace else None, "skipped", len(small))
        assert all(t <= F.CG_EPS / 100 for t in small), sorted(small)[-4:]


def test_a_nan_in_a_ray_or_pin_without_weight_is_never_used():
    case = Y.make_case("tree8", 1, 3, "rays")
    rng = np.random.default_rng(8)
    w = np.ones((8, 3), np.float32)
    w[3, 1], w[6, 0], w[6, 2] = 0.0, -1.0, np.nan
    pw = np.ones(8, np.float32)
    pw[[1, 5]] = [0.0, np.nan]
    pins = (case["goal"][0] + rng.normal(0, 0.01, (8, 3))).astype(np.float32)
    o, d = case["origins"][0].copy(), case["directions"][0].copy()
    args = (case["joints"], case["parents"], case["q0"][0], case["gt0"][0])
    base = Y.solve(*args, o, d, w, pins, pw, iterations=4, dtype=np.float32)
    o[w <= 0], d[w <= 0] = np.nan, np.nan
    o[6, 2], d[6, 2] = np.nan, np.nan
    pins[[1, 5]] = np.nan
    got = Y.solve(*args, o, d, w, pins, pw, iterations=4, dtype=np.float32)
    for k in KEYS:
        assert np.isfinite(got[k]).all() and np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), k
    # a zero or NaN direction switches its ray off: the problem without it
    d2, w2 = case["directions"][0].copy(), np.ones((8, 3), np.float32)
    d2[2, 0], d2[4, 1] = 0.0, np.nan
    w2[2, 0], w2[4, 1] = 0.0, 0.0
    a = Y.solve(*args, case["origins"][0], d2, None, iterations=4, dtype=np.float32)
    b = Y.solve(*args, case["origins"][0], case["directions"][0], w2, iterations=4, dtype=np.float32)
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("with_K", [False, True])
def test_camera_rays_inverts_the_pinhole(with_K):
    H, W = 120, 200
    cam = synth.look_at_camera(H, W, azimuth_deg=35.0, elevation_deg=15.0, radius=3.5, fovx=0.8, fovy=0.5)
    if with_K:
        fx, fy, _, _ = camera_intrinsics(cam)
        cam.K = [[fx, 0.0, 0.5 * W + 7.25], [0.0, fy, 0.5 * H - 3.5], [0.0, 0.0, 1.0]]
    fx, fy, cx, cy = camera_intrinsics(cam)
    assert (cx, cy) == ((0.5 * W + 7.25, 0.5 * H - 3.5) if with_K else (W / 2, H / 2))
    rng = np.random.default_rng(9)
    p = rng.uniform(-0.8, 0.8, (2, 50, 3))
    V = cam.world_view_transform.double().numpy()
    t = p @ V[:3, :3] + V[3, :3]  # csrc/pinhole.h: pinhole_view, pinhole_row_col
    xy = np.stack([fx * t[..., 0] / t[..., 2] + cx, fy * t[..., 1] / t[..., 2] + cy], -1)
    origin, directions = PE.camera_rays(cam, torch.from_numpy(xy.astype(np.float32)))
    assert origin.shape == (3,) and directions.shape == (2, 50, 3) and directions.dtype == torch.float32
    o, d = origin.double().numpy(), directions.double().numpy()
    assert np.abs(o - cam.camera_center.double().numpy()).max() <= 1e-5
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    v = p - o
    off = np.linalg.norm(v - (v * d).sum(-1, keepdims=True) * d, axis=-1)
    dist = np.linalg.norm(v, axis=-1)
    print("largest distance to the ray / distance to the camera", (off / dist).max())
    assert (off <= 1e-5 * dist).all()
    assert ((v * d).sum(-1) > 0).all()  # (in front of the camera, along +direction)


def test_refusals_that_need_no_device():
    case = Y.make_case("tree8", 1, 2)
    rig = (torch.from_numpy(case["joints"]), torch.from_numpy(case["parents"]))
    pose = {"local_rotation": torch.from_numpy(case["q0"][0]), "global_trans": torch.from_numpy(case["gt0"])}
    o, d = torch.from_numpy(case["origins"][0]), torch.from_numpy(case["directions"][0])
    for steps in (0, -3):
        with pytest.raises(L.RiggsHipError, match="cg_steps"):
            PE.fit_rays(rig, pose, o, d, cg_steps=steps)
    with pytest.raises(L.RiggsHipError, match="CUDA"):  # host tensors: no quiet CPU path
        PE.fit_rays(rig, pose, o, d)
    with pytest.raises(L.RiggsHipError, match="CUDA"):
        PE.fit_rays(rig, pose, None, None, pins=torch.from_numpy(case["goal"][0]))
    with pytest.raises(L.RiggsHipError, match="9 rays"):  # K > 8
        PE.fit_rays(rig, pose, torch.zeros(8, 9, 3), torch.ones(8, 9, 3))
    for bad_o, bad_d, kw in ((o[:, :1], d, {}), (o, d[..., :2], {}), (o.reshape(-1, 3), d, {}), (o, d.reshape(-1), {}),
                             (o, d, dict(weights=torch.ones(8, 3))), (o, d, dict(weights=torch.ones(8))),
                             (o, d, dict(pins=torch.zeros(8, 2))), (o, d, dict(pins=torch.zeros(8, 3), pin_weights=torch.ones(7))),
                             (o, None, {}), (None, None, {}), (None, None, dict(pin_weights=torch.ones(8))),
                             (None, None, dict(pins=torch.zeros(8, 3), weights=torch.ones(8, 2))), (o, d, dict(pin_weights=torch.ones(8)))):
        with pytest.raises(L.RiggsHipError) as err:
            PE.fit_rays(rig, pose, bad_o, bad_d, **kw)
        assert "CUDA" not in str(err.value), (kw, str(err.value))  # (refused for what it is, before any device is asked for)
    # the binding is the header's, and the C entry refuses before it launches (the addresses are never read)
    assert len(_abi.FUNCTIONS["riggs_fit_rays"][1]) == 25 and _abi.CONSTANTS["RIGGS_RAYS_MAX"] == 8 == Y.RAYS_MAX
    assert _abi.CONSTANTS["RIGGS_ABI_VERSION"] == 102
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(B=1, J=8, K=2, iterations=4, cg_steps=4, damping=0.1, max_step=1.0, extent=p, relative=0, rays=(p, p, p), pins=(None, None)):
        return L.lib().riggs_fit_rays(B, J, K, p, p, p, p, rays[0], rays[1], rays[2], pins[0], pins[1], None, iterations, cg_steps,
                                      damping, max_step, extent, relative, 0, p, p, p, p, None)
    for kw in (dict(B=0), dict(J=0), dict(J=257), dict(iterations=-1), dict(damping=0.0), dict(damping=float("nan")),
               dict(max_step=-1.0), dict(relative=4),                                                 # what solve_args refuses
               dict(K=-1), dict(K=9), dict(cg_steps=0), dict(extent=None),
               dict(rays=(None, p, p)), dict(rays=(p, None, p)), dict(rays=(p, p, None)),             # K > 0 with a NULL ray array
               dict(K=0, rays=(None, None, None)),                                                    # K == 0 without pins
               dict(pins=(p, None)), dict(pins=(None, p)), dict(K=0, rays=(None, None, None), pins=(p, None))):
        assert call(**kw) != 0, kw
        assert "riggs_fit_rays" in L.lib().riggs_last_error().decode(), kw
