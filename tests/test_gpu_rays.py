"""-m gpu: riggs_amd.pose_edit.fit_rays / fit_keypoints (csrc/rays.hip) against tests/rays_ref.py — float64 is the oracle, its
float32 form the yardstick for rounding.

Bars (those of tests/test_gpu_fit.py, for its reason).  PARITY per case, snapshot and tensor: max(8 * e32, 1e-6), e32 = the
float32 restatement's own deviation from float64 (positions, the translation and the residual relative to the rig's extent).
REACH: residual <= max(4 * r32, 1e-5 * extent) after 32 iterations, r32 the float32 restatement's residual.  With
RIGGS_RAYS_PARITY_JSON set to a path, what was measured is written there (profiles/rays_parity.json is such a record)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import pose_edit as PE  # noqa: E402
from riggs_amd import synth  # noqa: E402
from riggs_amd.loss import camera_intrinsics  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import ik_ref as R  # noqa: E402
from tests import rays_ref as Y  # noqa: E402
from tests.pose_solve_util import T, bits, deviation, make_rig, parity_bars, parity_report  # noqa: E402

COUNTS = Y.SNAPSHOTS
KEYS = ("local_rotation", "global_trans", "d_nodes", "residual")
POSE_KEYS = ("local_rotation", "global_trans", "d_nodes")
ARRAYS = ("origins", "directions", "weights", "pins", "pin_weights")
PARAMS = [(name, K, kind, B) for name, K, kind in Y.PARITY for B in (1, 3)]
IDS = ["%s-K%d-%s-B%d" % p for p in PARAMS]
# tests/test_gpu_fit.py's FEATURES, for its reason: what the solver's frame does in each of its two forms (one wave: two_joints;
# 256 threads: tree65) and no case above asks of it.  K = 2, 3 problems, FEATURE_COUNTS iterations, the bars of the cases above.
FEATURES = {"absolute": dict(damping=0.07, max_step=0.6), "max_step": dict(max_step=0.6), "damping": dict(damping=0.07),
            "translation": dict(solve_translation=True), "one_cg_step": dict(cg_steps=1), "cg_steps_over_J": dict(cg_steps=8)}
FEATURE_COUNTS = (1, 4)
FEATURE_PARAMS = [(name, 2, "rays", 3, f) for f in FEATURES for name in ("two_joints", "tree65")
                  if (name, f) not in (("two_joints", "one_cg_step"), ("tree65", "cg_steps_over_J"))]
_GPU, _REPORT = {}, {}
report = parity_report("RIGGS_RAYS_PARITY_JSON", _REPORT)


def run(case, iterations, **kw):
    """fit_rays on a case's batch -> numpy arrays (B, ...); keywords replace the case's own arrays."""
    pose = {"local_rotation": T(kw.pop("q0", case["q0"])), "global_trans": T(kw.pop("gt0", case["gt0"]))}
    arr = {k: kw.pop(k, case[k]) for k in ARRAYS}
    arr = {k: None if v is None else T(np.asarray(v, np.float32)) for k, v in arr.items()}
    if kw.get("locked") is not None:
        kw["locked"] = T(np.asarray(kw["locked"]))
    kw.setdefault("cg_steps", case["cg_steps"])
    kw.setdefault("solve_translation", case["solve_translation"])
    joints, parents = kw.pop("joints", case["joints"]), kw.pop("parents", case["parents"])
    out = PE.fit_rays((T(joints), T(parents)), pose, arr["origins"], arr["directions"], weights=arr["weights"], pins=arr["pins"],
                      pin_weights=arr["pin_weights"], iterations=iterations, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def reference(name, B, K=8, kind="rays", feature=None):
    """(case, float64 snapshots, float32 snapshots, GPU results) per iteration count: computed once, shared, never changed."""
    key = (name, B, K, kind, feature)
    if key not in _GPU:
        if feature is None:
            case, o64, o32 = Y.reference(name, B, K, kind)
            kw, counts = {}, COUNTS
        else:
            case, kw, counts = Y.make_case(name, B, K, kind), FEATURES[feature], FEATURE_COUNTS
            o64 = Y.solve_case(case, max(counts), np.float64, snapshots=counts, **kw)
            o32 = Y.solve_case(case, max(counts), np.float32, snapshots=counts, **kw)
        _GPU[key] = (case, o64, o32, {n: run(case, n, **kw) for n in counts})
    return _GPU[key]


def check_parity(label, extent, o64, o32, gpu):
    """Per snapshot: every tensor of ``gpu`` within max(8 * e32, 1e-6) of the float64 oracle; what was measured goes to the record."""
    failed = []
    for n in sorted(gpu):
        bar, e32 = parity_bars(o64[n], o32[n], KEYS, extent)
        dev = {k: deviation(gpu[n][k], o64[n][k], k, extent) for k in KEYS}
        _REPORT["%s-it%d" % (label, n)] = {"e32": e32, "gpu": dev, "bar": bar,
                                           "gpu_over_e32": {k: (dev[k] / e32[k] if e32[k] > 0 else None) for k in KEYS},
                                           "residual_over_extent": {"float64": float(o64[n]["residual"].max() / extent),
                                                                    "float32": float(o32[n]["residual"].max() / extent),
                                                                    "gpu": float(gpu[n]["residual"].max() / extent)}}
        print(label, n, "e32", e32, "gpu", dev)
        failed += ["%s after %d iterations: %.3g > %.3g (e32 %.3g)" % (k, n, dev[k], bar[k], e32[k]) for k in KEYS if not dev[k] <= bar[k]]
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("name,K,kind,B,feature", [p + (None,) for p in PARAMS] + FEATURE_PARAMS,
                         ids=IDS + ["%s-K%d-%s-B%d-%s" % p for p in FEATURE_PARAMS])
def test_parity_with_the_float64_oracle(name, K, kind, B, feature):
    case, o64, o32, gpu = reference(name, B, K, kind, feature)
    check_parity("-".join(filter(None, (name, "K%d" % K, kind, feature, "B%d" % B))), case["extent"], o64, o32, gpu)


def distances(case, d_nodes):
    """The largest distance of each returned joint to one of its lines (all weights 1, no pins), in float64."""
    o, d = case["origins"].astype(np.float64), case["directions"].astype(np.float64)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    v = o - d_nodes.astype(np.float64)[:, :, None, :]
    return np.linalg.norm(v - (v * d).sum(-1, keepdims=True) * d, axis=-1).max(-1)


@pytest.mark.parametrize("name,K,B", [(name, K, B) for name, K in Y.REACH for B in (1, 3)])
def test_reach(name, K, B):
    case, o64, o32, gpu = reference(name, B, K)
    r32 = np.asarray(o32[32]["residual"], np.float64)
    got = np.asarray(gpu[32]["residual"], np.float64)
    print(name, K, B, "residual / extent: gpu", got.max() / case["extent"], "float32", r32.max() / case["extent"])
    assert np.isfinite(got).all() and (got <= np.maximum(4 * r32, 1e-5 * case["extent"])).all(), (got, r32)
    # residual is the largest distance of the returned skeleton's joint to one of its lines (float32 positions about 4 extents
    # from the origins: their rounding, 4 extents * 2^-23, with a margin of 20)
    mine = distances(case, gpu[32]["d_nodes"])
    assert np.abs(mine - got).max() <= 1e-5 * case["extent"], np.abs(mine - got).max()


def subtree_table(case):
    return R.paths(case["parents"], np.arange(case["J"])).T  # [a, h]: h is in a's subtree


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_locked_joints_and_joints_with_nothing_constrained_below_them_keep_their_bits(name):
    case = Y.make_case(name, 3, 2)
    J = case["J"]
    below = subtree_table(case)
    a = max(range(1, J), key=lambda i: (min(int(below[i].sum()), 6), -i))  # a joint with a few joints below it
    assert below[a].sum() >= 2
    w = np.ones((J, 2), np.float32)
    w[below[a]] = 0  # no ray in a's subtree: nothing below a is observed
    locked = np.zeros(J, bool)
    locked[np.flatnonzero(~below[a])[1::2]] = True
    out = run(case, 8, weights=w, locked=locked)
    still = locked | below[a]
    assert np.array_equal(bits(out["local_rotation"][:, still]), bits(case["q0"][:, still]))
    moved = out["local_rotation"][:, ~still] != case["q0"][:, ~still]
    free = np.flatnonzero(~still)
    live = (w > 0).any(-1)
    has_ray_below = np.array([(below[i] & live & (np.arange(J) != 0)).any() for i in free])
    assert moved.any(-1)[:, has_ray_below].all()  # ... and every other joint with a ray to reach turned
    assert (out["residual"][:, below[a]] == 0).all() and np.isfinite(out["residual"]).all()


@pytest.mark.parametrize("name", ["root_only", "tree24", "tree256"])
def test_rays_through_the_current_posed_joints_change_nothing(name):
    case = Y.make_case(name, 3, 3)
    start = run(case, 0)  # no iteration: the forward kinematics of the starting pose
    assert np.array_equal(bits(start["local_rotation"]), bits(case["q0"])) and np.array_equal(bits(start["global_trans"]), bits(case["gt0"]))
    on_joints = np.repeat(start["d_nodes"][:, :, None, :], 3, 2)  # the origins ON the joints: e is exactly 0
    out = run(case, 8, origins=on_joints)
    for k in POSE_KEYS:
        assert np.array_equal(bits(out[k]), bits(start[k])), k
    assert (out["residual"] == 0).all()
    out = run(case, 8, origins=on_joints, pins=start["d_nodes"], pin_weights=np.ones((3, case["J"]), np.float32))
    for k in POSE_KEYS:
        assert np.array_equal(bits(out[k]), bits(start[k])), k
    assert (out["residual"] == 0).all()


def one_problem(case, b):
    return dict(case, B=1, q0=case["q0"][b:b + 1], gt0=case["gt0"][b:b + 1],
                **{k: (None if case[k] is None else case[k][b:b + 1]) for k in ARRAYS})


@pytest.mark.parametrize("name", ["tree24", "tree64", "tree256"])
def test_runs_are_bit_identical_and_problems_independent(name):
    case, _, _, gpu = reference(name, 3)
    again = run(case, 32)
    for k in KEYS:
        assert np.array_equal(bits(again[k]), bits(gpu[32][k])), k
    for b in range(case["B"]):
        alone = run(one_problem(case, b), 32)
        for k in KEYS:
            assert np.array_equal(bits(alone[k][0]), bits(gpu[32][k][b])), (k, b)


@pytest.mark.parametrize("name,K,kind", [("tree24", 3, "mixed"), ("tree65", 3, "mixed"), ("tree64", 8, "rays")])
def test_rays_read_again_in_every_iteration_give_the_same_bits(name, K, kind):
    """riggs_set_option("rays_reread", 1): the rays from global memory in every iteration instead of from registers."""
    case, _, _, gpu = reference(name, 3, K, kind)
    try:
        L.set_option("rays_reread", 1)
        other = run(case, 32)
    finally:
        L.set_option("rays_reread", 0)
    for k in KEYS:
        assert np.array_equal(bits(other[k]), bits(gpu[32][k])), k


def test_wave_form_and_workgroup_form_give_the_same_bits():
    """tree64 with one more leaf without any constraint (J = 65: 256 threads, the sweeps through LDS) against the 64-joint problem
    on one wave: BIT-IDENTICAL, for tests/test_gpu_fit.py's reason (the order of every sum is the same)."""
    name, B, K = "tree64", 3, 8
    case, _, _, gpu = reference(name, B)
    joints = np.concatenate([case["joints"], 0.5 * (case["joints"][0:1] + case["joints"][1:2])]).astype(np.float32)  # (inside the box: same extent)
    assert R.extent_of(joints) == R.extent_of(case["joints"])
    parents = np.concatenate([case["parents"], [0]]).astype(np.int32)
    q0 = np.concatenate([case["q0"], np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1, 1))], 1)
    junk = np.full((B, 1, K, 3), np.nan, np.float32)
    w = np.ones((B, 65, K), np.float32)
    w[:, 64] = 0
    wide = run(case, 32, joints=joints, parents=parents, q0=q0, origins=np.concatenate([case["origins"], junk], 1),
               directions=np.concatenate([case["directions"], junk], 1), weights=w)
    for k in KEYS:
        a = wide[k][:, :64] if k != "global_trans" else wide[k]
        assert np.array_equal(bits(a), bits(gpu[32][k])), k
    assert np.array_equal(bits(wide["local_rotation"][:, 64]), bits(q0[:, 64])) and (wide["residual"][:, 64] == 0).all()


def test_eight_rays_with_five_of_weight_zero_give_the_bits_of_three():
    case = Y.make_case("tree24", 3, 3)
    three = run(case, 8)
    B, J = 3, case["J"]
    o, d = np.full((B, J, 8, 3), np.nan, np.float32), np.full((B, J, 8, 3), np.nan, np.float32)
    w = np.zeros((B, J, 8), np.float32)
    slots = [1, 4, 6]
    o[:, :, slots], d[:, :, slots], w[:, :, slots] = case["origins"], case["directions"], 1
    eight = run(case, 8, origins=o, directions=d, weights=w)
    for k in KEYS:
        assert np.isfinite(eight[k]).all() and np.array_equal(bits(eight[k]), bits(three[k])), k


def test_junk_in_constraints_without_weight_changes_no_bit():
    case = Y.make_case("tree24", 3, 3, "mixed")
    n = 8
    got = run(case, n)
    w, pw = case["weights"], case["pin_weights"]
    none = (w <= 0).all(-1) & (pw <= 0)
    assert none.any() and (got["residual"][none] == 0).all() and (got["residual"][~none] > 0).all()
    for junk in (np.nan, np.inf, 1e30):
        o, d, pins = case["origins"].copy(), case["directions"].copy(), case["pins"].copy()
        o[w <= 0], d[w <= 0], pins[pw <= 0] = junk, junk, junk
        other = run(case, n, origins=o, directions=d, pins=pins)
        for k in KEYS:
            assert np.isfinite(other[k]).all() and np.array_equal(bits(other[k]), bits(got[k])), (junk, k)
    for bad in (-1.0, float("nan")):  # a negative and a NaN weight switch off as well
        w2, pw2 = w.copy(), pw.copy()
        w2[w <= 0], pw2[pw <= 0] = bad, bad
        other = run(case, n, weights=w2, pin_weights=pw2)
        for k in KEYS:
            assert np.array_equal(bits(other[k]), bits(got[k])), (bad, k)
    for bad in (0.0, float("nan"), float("inf")):  # a zero, NaN or infinite direction switches its ray off, whatever its weight
        d2, w2 = case["directions"].copy(), w.copy()
        d2[w <= 0] = bad
        w2[w <= 0] = 1.5
        other = run(case, n, directions=d2, weights=w2)
        for k in KEYS:
            assert np.array_equal(bits(other[k]), bits(got[k])), (bad, k)


# --------------------------------------------------------------------------- keypoints
def project64(cam, points):
    """csrc/pinhole.h's rule in float64: (..., 3) world points -> (..., 2) as (x, y) = (column, row)."""
    fx, fy, cx, cy = camera_intrinsics(cam)
    V = cam.world_view_transform.double().cpu().numpy()
    t = np.asarray(points, np.float64) @ V[:3, :3] + V[3, :3]
    return np.stack([fx * t[..., 0] / t[..., 2] + cx, fy * t[..., 1] / t[..., 2] + cy], -1)


def test_fit_keypoints_is_fit_rays_on_camera_rays():
    H, W, B = 300, 400, 3
    case = Y.make_case("tree24", B, 2)
    J = case["J"]
    cams = [synth.look_at_camera(H, W, azimuth_deg=az, elevation_deg=10.0, radius=4.0) for az in (20.0, 110.0)]
    kp = np.stack([project64(c, case["goal"]) for c in cams], 1).astype(np.float32)  # (B, C, J, 2)
    conf = np.random.default_rng(4).uniform(0.3, 1.0, (B, 2, J)).astype(np.float32)
    conf[0, 0, 5], conf[1, 1, 7], conf[2, :, 9] = 0.0, -1.0, 0.0
    rig = (T(case["joints"]), T(case["parents"]))
    pose = {"local_rotation": T(case["q0"]), "global_trans": T(case["gt0"])}
    out = PE.fit_keypoints(rig, pose, cams, T(kp), weights=T(conf), iterations=8)
    assert out["reprojection"].shape == (B, 2, J) and out["d_nodes"].shape == (B, J, 3)
    rays = [PE.camera_rays(c, T(kp)[:, i]) for i, c in enumerate(cams)]
    direct = PE.fit_rays(rig, pose, torch.stack([o for o, _ in rays]), torch.stack([d for _, d in rays], 2),
                         weights=T(conf).transpose(1, 2), iterations=8)
    for k in KEYS:
        assert torch.equal(out[k], direct[k]), k
    want = np.stack([np.linalg.norm(project64(c, out["d_nodes"].cpu().numpy()) - kp[:, i].astype(np.float64), axis=-1)
                     for i, c in enumerate(cams)], 1)
    want[conf <= 0] = 0
    got = out["reprojection"].cpu().numpy()
    print("reprojection: largest", want.max(), "px; largest difference to float64", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-5 * max(W, H) and (got[conf <= 0] == 0).all()
    # an unseen keypoint may hold anything
    kp2 = kp.copy()
    kp2[conf <= 0] = np.nan
    other = PE.fit_keypoints(rig, pose, cams, T(kp2), weights=T(conf), iterations=8)
    for k in KEYS + ("reprojection",):
        assert torch.equal(other[k], out[k]) and bool(torch.isfinite(other[k]).all()), k
    # unbatched: one frame
    single = PE.fit_keypoints(rig, {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"][0:1])}, cams, T(kp[0]),
                              weights=T(conf[0]), iterations=8)
    assert single["reprojection"].shape == (2, J) and torch.equal(single["local_rotation"], out["local_rotation"][0])


def test_the_editors_drag():
    """One camera: the cursor's ray on a leaf joint, pins at the current posed joints on every joint off the leaf's root path."""
    H = W = 400
    case = Y.make_case("tree24", 1, 1)
    J, ext = case["J"], case["extent"]
    cam = synth.look_at_camera(H, W, azimuth_deg=30.0, elevation_deg=15.0, radius=4.0)
    rig = (T(case["joints"]), T(case["parents"]))
    pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"])}
    leaf = int(R.deepest(case["parents"], 1)[0])
    on_path = R.paths(case["parents"], [leaf])[0]
    start = run(case, 0)["d_nodes"][0]
    kp = project64(cam, start).astype(np.float32)[None]          # (1, J, 2)
    kp[0, leaf] += np.array([40.0, -25.0], np.float32)
    conf = np.zeros((1, J), np.float32)
    conf[0, leaf] = 1
    pw = (~on_path).astype(np.float32)
    counts = (1, 8, 32)
    gpu = {}
    for n in counts:
        out = PE.fit_keypoints(rig, pose, [cam], T(kp), weights=T(conf), pins=T(start), pin_weights=T(pw), iterations=n)
        gpu[n] = {k: out[k].cpu().numpy()[None] if k != "global_trans" else out[k].cpu().numpy() for k in KEYS}
    origin, directions = PE.camera_rays(cam, T(kp))
    o = np.broadcast_to(origin.cpu().numpy(), (J, 1, 3))
    d = directions.cpu().numpy().transpose(1, 0, 2)              # (J, 1, 3)
    args = (case["joints"], case["parents"], case["q0"][0], case["gt0"][0], o, d, conf.T, start, pw)
    stack = lambda snaps: {n: {k: v[None] for k, v in snaps[n].items()} for n in counts}  # noqa: E731
    o64 = stack(Y.solve(*args, iterations=32, snapshots=counts))
    o32 = stack(Y.solve(*args, iterations=32, snapshots=counts, dtype=np.float32))
    check_parity("editor_drag-tree24", ext, o64, o32, gpu)
    r32, got = float(o32[32]["residual"][0, leaf]), float(gpu[32]["residual"][0, leaf])
    print("leaf residual / extent: gpu", got / ext, "float32", r32 / ext, "pinned joints moved by", gpu[32]["residual"][0, ~on_path].max() / ext)
    assert got <= max(4 * r32, 1e-5 * ext)


def test_unreachable_rays_stay_finite_and_translation_brings_them_back():
    shift = lambda case: (case["origins"] + np.float32(10 * case["extent"]) * np.array([0.6, 0.0, 0.8], np.float32)).astype(np.float32)  # noqa: E731
    for name in ("chain4", "tree8", "tree256"):
        case = Y.make_case(name, 3, 2)
        for n in (8, 32):
            out = run(case, n, origins=shift(case))
            assert all(np.isfinite(out[k]).all() for k in out), (name, n)
    case = Y.make_case("tree8", 3, 8)
    ext, far = case["extent"], shift(case)
    r32 = np.asarray(Y.solve_case(case, 32, np.float32, origins=far, solve_translation=True)["residual"], np.float64)
    got = np.asarray(run(case, 32, origins=far, solve_translation=True)["residual"], np.float64)
    print("tree8 shifted by 10 extents, solve_translation: residual / extent gpu", got.max() / ext, "float32", r32.max() / ext)
    assert np.isfinite(got).all() and (got <= np.maximum(4 * r32, 1e-5 * ext)).all(), (got, r32)


@pytest.mark.parametrize("name", ["tree24", "tree65"])
def test_the_pose_goes_through_the_rig(name):
    case = Y.make_case(name, 3, 2)
    sw, x = make_rig(case)
    mask = torch.ones(x.shape[0], 1, device="cuda")
    pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"][0:1])}
    o, d = T(case["origins"]), T(case["directions"])
    out = PE.fit_rays(sw, pose, o[0], d[0], iterations=8)
    assert out["local_rotation"].shape == (case["J"], 4) and out["global_trans"].shape == (1, 3)
    assert out["d_nodes"].shape == (case["J"], 3) and out["residual"].shape == (case["J"],)
    dd = sw.deform_by_pose(x, out, mask)
    U.assert_close(dd["d_nodes"].detach().cpu().numpy(), out["d_nodes"].cpu().numpy(), "d_nodes of the fitted pose through deform_by_pose", 1e-5)
    same = PE.fit_rays((T(case["joints"]), case["parents"]), pose, o[0, 0], d[0], iterations=8)  # host parents, (K, 3) origins
    assert torch.equal(same["local_rotation"], out["local_rotation"])
    # a clip -> a pose track: the (B, J, 4) result feeds deform_sequence unchanged
    track = PE.fit_rays(sw, {"local_rotation": T(case["q0"]), "global_trans": T(case["gt0"])}, o, d, iterations=8)
    assert track["local_rotation"].shape == (3, case["J"], 4) and track["global_trans"].shape == (3, 3)
    assert torch.equal(track["local_rotation"][0], out["local_rotation"])
    seq = sw.deform_sequence(x, track, mask)
    U.assert_close(seq["d_nodes"].cpu().numpy(), track["d_nodes"].cpu().numpy(), "d_nodes of the fitted track through deform_sequence", 1e-5)
    # pins alone (K = 0) are fit_pose's problem: the same kinematics, its own rounding of s * (s * r) against w * r
    pinned = PE.fit_rays(sw, pose, None, None, pins=T(case["goal"][0]), iterations=8)
    fitted = PE.fit_pose(sw, pose, T(case["goal"][0]), iterations=8)
    U.assert_close(pinned["d_nodes"].cpu().numpy(), fitted["d_nodes"].cpu().numpy(), "pins alone against fit_pose", 1e-4)


def test_capture_and_replay():
    H, W = 300, 400
    case = Y.make_case("tree24", 1, 2)
    sw, x = make_rig(case)
    mask = torch.ones(x.shape[0], 1, device="cuda")
    cams = [synth.look_at_camera(H, W, azimuth_deg=az, elevation_deg=10.0, radius=4.0).to("cuda") for az in (20.0, 110.0)]
    q0, gt0 = T(case["q0"][0]), T(case["gt0"])
    kp = T(np.stack([project64(c, case["goal"][0]) for c in cams]).astype(np.float32))
    conf = torch.ones(2, case["J"], device="cuda")

    @torch.no_grad()
    def step():
        out = PE.fit_keypoints(sw, {"local_rotation": q0, "global_trans": gt0}, cams, kp, weights=conf, iterations=8)
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
        kp.add_(3.0 * torch.randn(kp.shape, generator=g).cuda())
        if rep == 1:
            conf[1, 5] = 0.0
            kp[1, 5] = float("nan")
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_xyz = step()
        for k in eager:
            assert torch.equal(eager[k], out[k]), (rep, k)
        U.assert_close(d_xyz.cpu().numpy(), eager_xyz.cpu().numpy(), "d_xyz of the replay", 1e-6)


def test_refusals():
    case = Y.make_case("tree24", 3, 2)
    J = case["J"]
    rig = (T(case["joints"]), T(case["parents"]))
    pose = {"local_rotation": T(case["q0"][0]), "global_trans": T(case["gt0"][0:1])}
    o, d = T(case["origins"][0]), T(case["directions"][0])
    for steps in (0, -1):
        with pytest.raises(L.RiggsHipError):
            PE.fit_rays(rig, pose, o, d, cg_steps=steps)
    for damping in (0.0, -0.1, float("nan")):
        with pytest.raises(L.RiggsHipError):
            PE.fit_rays(rig, pose, o, d, damping=damping)
    with pytest.raises(L.RiggsHipError):
        PE.fit_rays(rig, pose, o, d, max_step=-1.0)
    with pytest.raises(L.RiggsHipError):
        PE.fit_rays(rig, pose, o, d, iterations=-1)
    for bad_o, bad_d in ((o[:-1], d[:-1]), (o, d[:, :1]), (o[:, 0], d[:, 0]), (o, d[..., :2]), (o.cpu(), d), (o, d.cpu())):
        with pytest.raises(L.RiggsHipError):
            PE.fit_rays(rig, pose, bad_o, bad_d)
    with pytest.raises(L.RiggsHipError):  # K > 8
        PE.fit_rays(rig, pose, torch.zeros(J, 9, 3, device="cuda"), torch.ones(J, 9, 3, device="cuda"))
    for kw in (dict(weights=torch.ones(J, 3, device="cuda")), dict(weights=torch.ones(J, 2)), dict(pins=torch.zeros(J - 1, 3, device="cuda")),
               dict(pins=torch.zeros(J, 3)), dict(pin_weights=torch.ones(J, device="cuda")),
               dict(pins=torch.zeros(J, 3, device="cuda"), pin_weights=torch.ones(J + 1, device="cuda")),
               dict(locked=torch.zeros(J + 1, dtype=torch.bool))):
        with pytest.raises(L.RiggsHipError):
            PE.fit_rays(rig, pose, o, d, **kw)
    with pytest.raises(L.RiggsHipError):  # mismatched batch sizes
        PE.fit_rays(rig, {"local_rotation": T(case["q0"]), "global_trans": T(case["gt0"])}, T(case["origins"][:2]), T(case["directions"][:2]))
    with pytest.raises(L.RiggsHipError):  # neither rays nor pins
        PE.fit_rays(rig, pose, None, None)
    cam = synth.look_at_camera(100, 100)
    with pytest.raises(L.RiggsHipError):  # 9 cameras
        PE.fit_keypoints(rig, pose, [cam] * 9, torch.zeros(9, J, 2, device="cuda"))
    with pytest.raises(L.RiggsHipError):
        PE.fit_keypoints(rig, pose, [cam], torch.zeros(2, J, 2, device="cuda"))
    with pytest.raises(L.RiggsHipError):  # no quiet CPU path
        PE.fit_keypoints(rig, pose, [cam], torch.zeros(1, J, 2))
    # the C entry refuses the same on its own: nothing is launched (the outputs keep their fill)
    out, buf = U.out_buf((J, 4))
    z = torch.zeros(4 * 257 * 8, device="cuda")
    ext = torch.ones(1, device="cuda")
    zp = z.data_ptr()
    ok = dict(Jc=J, K=2, steps=4, damping=0.1, e=ext, rays=(zp, zp, zp), pins=(None, None))
    for change in (dict(Jc=0), dict(Jc=257), dict(K=9), dict(K=-1), dict(steps=0), dict(damping=0.0), dict(e=None),
                   dict(rays=(None, zp, zp)), dict(rays=(zp, zp, None)), dict(K=0, rays=(None, None, None)),
                   dict(pins=(zp, None)), dict(pins=(None, zp))):
        c = dict(ok, **change)
        rc = L.lib().riggs_fit_rays(1, c["Jc"], c["K"], rig[0].data_ptr(), rig[1].data_ptr(), pose["local_rotation"].data_ptr(), zp,
                                    c["rays"][0], c["rays"][1], c["rays"][2], c["pins"][0], c["pins"][1], None, 4, c["steps"],
                                    c["damping"], 1.0, L.ptr(c["e"]), 0, 0, out.data_ptr(), zp, zp, zp, L.stream_ptr())
        assert rc != 0 and "riggs_fit_rays" in L.lib().riggs_last_error().decode(), change
    torch.cuda.synchronize()
    assert bool((buf == U.SENT).all())
