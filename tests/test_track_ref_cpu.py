"""Pose-track filtering without a GPU: the conditioning of every test case (the chordal mean is well defined where the second
eigenvalue stays far below the first), analytic properties of the float64 oracle (tests/track_ref.py), the float32 restatement
against it, the entry points in the header, and what ``smooth_track`` / ``one_euro_track`` refuse before any launch."""
import numpy as np
import pytest
import torch

from riggs_amd import _lib as L
from riggs_amd import track as TR
from tests import track_ref as R

SYMBOLS = ("riggs_track_smooth", "riggs_track_one_euro")


def test_every_case_is_well_conditioned():
    """lambda_2 / lambda_1 <= 0.25 wherever a window has support, on EVERY case of the GPU tests and of the experiment behind the
    sweep count (T = 48, J = 6, (sigma, R) in (1, 3), (2, 6), (5, 15))."""
    worst = {}
    for case in R.CASES:
        _, o64, _ = R.case_reference(case)
        ratio = o64["ratio"][o64["support"] > 0]
        worst[case["name"]] = float(ratio.max()) if ratio.size else 0.0
    print(worst)
    assert all(v <= 0.25 for v in worst.values()), {k: v for k, v in worst.items() if not v <= 0.25}
    assert {(c["sigma"], c["R"]) for c in R.CASES if c["T"] == 48} == {(1.0, 3), (2.0, 6), (5.0, 15)}


def test_the_float32_restatement_stays_next_to_the_oracle():
    """Four Jacobi sweeps in float32: within 5e-6 rad of eigh in float64 on every case (float32's epsilon over the smallest
    eigenvalue gap the conditioning bound allows, 1.2e-7 / 0.75, times a window's worth of roundings), supports to 1e-6."""
    for case in R.CASES:
        _, o64, o32 = R.case_reference(case)
        err = float(R.rotation_angle(o32["local_rotation"], o64["local_rotation"]).max())
        assert err <= 5e-6, (case["name"], err)
        assert np.abs(o32["support"] - o64["support"]).max() <= 1e-6 * max(1.0, o64["support"].max()), case["name"]
        assert np.abs(np.linalg.norm(o32["local_rotation"].astype(np.float64), axis=-1) - 1).max() <= 1e-6


def _smooth64(rot, **kw):
    return R.smooth(np.asarray(rot, np.float32)[None], None, dtype=np.float64, **kw)


def test_a_constant_rotation_comes_back():
    rng = np.random.default_rng(3)
    q = rng.standard_normal((1, 5, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    rot = q * (rng.choice([-1.0, 1.0], (30, 5)) * rng.uniform(0.5, 2.0, (30, 5)))[..., None]
    w = rng.uniform(0.1, 1.0, (30, 5)).astype(np.float32)
    out = _smooth64(rot, sigma=2.0, weights=w[None])
    assert R.rotation_angle(out["local_rotation"][0], np.broadcast_to(q, (30, 5, 4))).max() <= 1e-6  # (the inputs are float32)
    # ... in the hemisphere of each frame's own sample
    assert (R.dot4(out["local_rotation"][0], rot) >= 0).all()


def test_constant_angular_velocity_is_a_fixed_point_inside_the_track():
    rng = np.random.default_rng(4)
    T, Rr = 40, 6
    axis = rng.standard_normal(3)
    start = rng.standard_normal(4)
    start /= np.linalg.norm(start)
    q = R.quat_mul(start[None], R.axis_angle_quat(np.broadcast_to(axis, (T, 3)), 0.15 * np.arange(T)))[:, None]
    out = _smooth64(q, sigma=2.0, radius=Rr)
    err = R.rotation_angle(out["local_rotation"][0], q)
    assert err[Rr:T - Rr].max() <= 1e-6 and err[0].max() > 1e-3  # (the clipped window at the ends is one-sided)


def test_radius_zero_is_the_identity():
    tr = R.make_track(1, 9, 4, 5)
    for dtype in (np.float64, np.float32):
        out = R.smooth(tr["rot"], tr["trans"], 1.0, radius=0, weights=tr["weights"], dtype=dtype)
        want = tr["rot"].astype(np.float64) / np.linalg.norm(tr["rot"].astype(np.float64), axis=-1, keepdims=True)
        assert R.rotation_angle(out["local_rotation"], want).max() <= (1e-12 if dtype is np.float64 else 2e-6)
        assert (R.dot4(out["local_rotation"], want) > 0).all()
        gap = tr["weights"] <= 0
        assert gap.any() and (out["support"][gap] == 0).all() and np.allclose(out["support"][~gap], tr["weights"][~gap])


def test_a_fully_gapped_joint_reports_no_support_and_returns_its_input():
    tr = R.make_track(1, 12, 3, 6)
    tr["weights"][:, :, 1] = 0
    tr["rot"][0, 4, 1] = 0       # a zero and a NaN sample inside the gap: the identity there
    tr["rot"][0, 7, 1, 2] = np.nan
    out = R.smooth(tr["rot"], tr["trans"], 2.0, weights=tr["weights"], trans_weights=np.zeros((1, 12), np.float32))
    assert (out["support"][0, :, 1] == 0).all() and (out["support"][0, :, 0] > 0).all()
    keep = np.array([t not in (4, 7) for t in range(12)])
    want = tr["rot"][0, keep, 1].astype(np.float64)
    want = want / np.linalg.norm(want, axis=-1, keepdims=True)
    assert np.abs(out["local_rotation"][0, keep, 1] - want).max() <= 1e-15
    assert (out["local_rotation"][0, [4, 7], 1] == np.array([1.0, 0, 0, 0])).all()
    assert np.isfinite(out["local_rotation"]).all()
    assert np.array_equal(out["global_trans"], tr["trans"].astype(np.float64))  # no support: the input rows


def test_one_euro_holds_a_constant_track_and_follows_with_a_large_cutoff():
    rng = np.random.default_rng(7)
    q = rng.standard_normal((1, 1, 5, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    rot = np.broadcast_to(q, (1, 20, 5, 4)) * (rng.choice([-1.0, 1.0], (1, 20, 5)) * rng.uniform(0.5, 2.0, (1, 20, 5)))[..., None]
    trans = np.broadcast_to(rng.standard_normal((1, 1, 3)), (1, 20, 3))
    out = R.one_euro(rot, trans, 30.0, min_cutoff=1.0, beta=0.0)
    assert R.rotation_angle(out["local_rotation"], np.broadcast_to(q, (1, 20, 5, 4))).max() <= 1e-6
    assert np.abs(out["global_trans"] - trans).max() <= 1e-6
    tr = R.make_track(1, 20, 5, 8, gaps=0.0)
    out = R.one_euro(tr["rot"], tr["trans"], 30.0, min_cutoff=1e7, beta=0.0)
    want = tr["rot"].astype(np.float64)
    assert R.rotation_angle(out["local_rotation"], want).max() <= 1e-4 and np.abs(out["global_trans"] - tr["trans"]).max() <= 1e-4
    # a gap frame holds the last output; before the first sample the identity
    w = np.ones((1, 20, 5), np.float32)
    w[0, 0] = 0
    w[0, 9:12, 2] = 0
    out = R.one_euro(tr["rot"], tr["trans"], 30.0, weights=w)
    assert (out["local_rotation"][0, 0] == np.array([1.0, 0, 0, 0])).all()
    assert all(np.array_equal(out["local_rotation"][0, t, 2], out["local_rotation"][0, 8, 2]) for t in (9, 10, 11))
    assert (out["state"]["gap"] == 0).all()


def test_one_euro_in_two_calls_is_one_euro_in_one():
    tr = R.euro_track(2, 5, 9)
    args = dict(weights=tr["weights"], trans_weights=tr["trans_weights"], **R.EURO)
    for dtype in (np.float64, np.float32):
        whole = R.one_euro(tr["rot"], tr["trans"], dtype=dtype, **args)
        a = R.one_euro(tr["rot"][:, :17], tr["trans"][:, :17], dtype=dtype, **dict(args, weights=tr["weights"][:, :17], trans_weights=tr["trans_weights"][:, :17]))
        b = R.one_euro(tr["rot"][:, 17:], tr["trans"][:, 17:], dtype=dtype, state=a["state"],
                       **dict(args, weights=tr["weights"][:, 17:], trans_weights=tr["trans_weights"][:, 17:]))
        for k in ("local_rotation", "global_trans"):
            assert np.array_equal(np.concatenate([a[k], b[k]], 1), whole[k]), k
        assert whole["local_rotation"].dtype == dtype


def test_header_declares_the_entry_points_and_the_binding_has_their_signatures():
    assert set(SYMBOLS) <= set(L.exported_symbols())
    assert L.CONSTANTS["RIGGS_TRACK_MAX_RADIUS"] == R.MAX_RADIUS == TR.MAX_RADIUS and L.CONSTANTS["RIGGS_TRACK_MAX_JOINTS"] == R.MAX_JOINTS
    assert L.CONSTANTS["RIGGS_ABI_VERSION"] == 102  # added symbols: unchanged


def test_taps_are_float64_on_the_host_rounded_once():
    Rr, g = TR.gaussian_taps(2.0)
    assert Rr == 6 and g[0] == 1.0 and np.array_equal(np.asarray(g, np.float64).astype(np.float32), R.taps(2.0)[1])
    assert TR.gaussian_taps(0.4)[0] == 2 and TR.gaussian_taps(5.0, 3)[0] == 3 and TR.gaussian_taps(21.3)[0] == 64


# ------------------------------------------------------------------------------------------------ the host logic
@pytest.fixture
def launches(monkeypatch):
    """The two launches replaced by the restatement on CPU tensors, the device requirement lifted: what is checked is which
    tensors reach a launch, what is returned, and that a refusal comes before any launch."""
    seen = []
    N = lambda t: None if t is None else t.numpy()  # noqa: E731

    def smooth(B, T, J, Rr, wrap, rot, trans, weights, trans_weights, taps, rot_out, trans_out, support):
        seen.append(("smooth", B, T, J, Rr, wrap))
        assert tuple(rot.shape) == (B, T, J, 4) and tuple(taps.shape) == (Rr + 1,) and taps.dtype is torch.float32
        out = R.smooth(N(rot), N(trans), None, Rr, N(weights), N(trans_weights), wrap, np.float32, g=taps.numpy())
        rot_out.copy_(torch.from_numpy(out["local_rotation"]))
        support.copy_(torch.from_numpy(out["support"]))
        if trans is not None:
            trans_out.copy_(torch.from_numpy(out["global_trans"]))

    def euro(B, T, J, rot, trans, weights, trans_weights, params, state, rot_out, trans_out):
        seen.append(("euro", B, T, J))
        keys = ("rate", "min_cutoff", "beta", "d_cutoff", "trans_min_cutoff", "trans_beta")
        out = R.one_euro(N(rot), N(trans), weights=N(weights), trans_weights=N(trans_weights), dtype=np.float32,
                         state={k: v.numpy() for k, v in state.items()}, **dict(zip(keys, params)))
        rot_out.copy_(torch.from_numpy(out["local_rotation"]))
        if trans is not None:
            trans_out.copy_(torch.from_numpy(out["global_trans"]))
        for k in state:
            state[k].copy_(torch.from_numpy(out["state"][k]))
    monkeypatch.setattr(TR, "_smooth_launch", smooth)
    monkeypatch.setattr(TR, "_euro_launch", euro)
    monkeypatch.setattr(L, "require_cuda_f32", lambda name, t, shape=None: t)
    return seen


def _dict(tr, b=None):
    pick = (lambda a: torch.from_numpy(a)) if b is None else (lambda a: torch.from_numpy(a[b]))
    return {"local_rotation": pick(tr["rot"]), "global_trans": pick(tr["trans"]), "d_nodes": torch.zeros(3), "residual": torch.zeros(2)}


def test_what_goes_in_and_what_comes_back(launches):
    tr = R.make_track(2, 9, 4, 11)
    ref = R.smooth(tr["rot"], tr["trans"], 1.0, None, tr["weights"], tr["trans_weights"], False, np.float32)
    out = TR.smooth_track(_dict(tr), 1.0, weights=torch.from_numpy(tr["weights"]), trans_weights=torch.from_numpy(tr["trans_weights"]))
    assert launches == [("smooth", 2, 9, 4, 3, False)]
    assert sorted(out) == ["global_trans", "local_rotation", "local_rotation2", "num", "support"]  # no d_nodes, no residual
    assert out["local_rotation"] is out["local_rotation2"] and out["num"] == 9
    assert np.array_equal(out["local_rotation"].numpy(), ref["local_rotation"]) and np.array_equal(out["support"].numpy(), ref["support"])
    assert np.array_equal(out["global_trans"].numpy(), ref["global_trans"])
    # one track, (T, 1, 3) translations, the reference's name for the rotations
    one = _dict(tr, 1)
    one = {"local_rotation2": one["local_rotation"], "global_trans": one["global_trans"][:, None]}
    out1 = TR.smooth_track(one, 1.0, weights=torch.from_numpy(tr["weights"][1]), trans_weights=torch.from_numpy(tr["trans_weights"][1]))
    assert out1["local_rotation"].shape == (9, 4, 4) and out1["global_trans"].shape == (9, 3) and out1["support"].shape == (9, 4)
    assert np.array_equal(out1["local_rotation"].numpy(), ref["local_rotation"][1])  # (a track does not see the rest of the batch)
    # one translation for the whole track passes through untouched
    const = torch.randn(1, 3)
    outc = TR.smooth_track({"local_rotation": one["local_rotation2"], "global_trans": const}, 1.0)
    assert outc["global_trans"] is const and outc["num"] == 9
    # the one-euro filter: the state comes back, the one passed in is left alone; OneEuroTrack updates its own in place
    eo = TR.one_euro_track(_dict(tr), 30.0, beta=0.3)
    assert sorted(eo) == ["global_trans", "local_rotation", "local_rotation2", "num", "state"] and sorted(eo["state"]) == sorted(TR.STATE_KEYS)
    before = {k: v.clone() for k, v in eo["state"].items()}
    eo2 = TR.one_euro_track(_dict(tr), 30.0, beta=0.3, state=eo["state"])
    assert all(torch.equal(before[k], eo["state"][k]) for k in before) and eo2["state"]["rotation"] is not eo["state"]["rotation"]
    f = TR.OneEuroTrack(4, 30.0, beta=0.3, device="cpu")
    held = f.state["rotation"]
    got = [f.filter({"local_rotation": torch.from_numpy(tr["rot"][0, t]), "global_trans": torch.from_numpy(tr["trans"][0, t:t + 1])}) for t in range(9)]
    assert f.state["rotation"] is held and got[0]["local_rotation"].shape == (4, 4) and got[0]["global_trans"].shape == (1, 3)
    assert np.array_equal(torch.stack([g["local_rotation"] for g in got]).numpy(), eo["local_rotation"][0].numpy())
    f.reset()
    assert f.state["rotation"] is held and int(f.state["gap"].max()) == -1


def test_refusals_come_before_any_launch(launches):
    tr = R.make_track(1, 9, 4, 12)
    track = _dict(tr, 0)
    with pytest.raises(ValueError):  # R > 64
        TR.smooth_track(track, 2.0, radius=65)
    with pytest.raises(ValueError):
        TR.smooth_track(track, 22.0)
    with pytest.raises(ValueError):  # wrap with 2R + 1 > T
        TR.smooth_track(track, 2.0, radius=5, wrap=True)
    with pytest.raises(ValueError):
        TR.smooth_track(track, float("nan"))
    big = {"local_rotation": torch.ones(2, 257, 4), "global_trans": torch.zeros(2, 3)}
    with pytest.raises(L.RiggsHipError):  # J > 256
        TR.smooth_track(big, 1.0)
    with pytest.raises(L.RiggsHipError):
        TR.one_euro_track(big, 30.0)
    with pytest.raises(L.RiggsHipError):
        TR.OneEuroTrack(257, 30.0, device="cpu")
    for w in (torch.ones(9, 3), torch.ones(8, 4), torch.ones(1, 9, 4), torch.ones(36)):  # a weights shape that does not match
        with pytest.raises(L.RiggsHipError):
            TR.smooth_track(track, 1.0, weights=w)
        with pytest.raises(L.RiggsHipError):
            TR.one_euro_track(track, 30.0, weights=w)
    with pytest.raises(L.RiggsHipError):
        TR.smooth_track(track, 1.0, trans_weights=torch.ones(8))
    with pytest.raises(L.RiggsHipError):
        TR.smooth_track({"local_rotation": track["local_rotation"], "global_trans": torch.zeros(4, 3)}, 1.0)
    for bad in (dict(rate=0.0), dict(rate=30.0, min_cutoff=0.0), dict(rate=30.0, beta=-1.0), dict(rate=30.0, d_cutoff=float("inf"))):
        with pytest.raises(ValueError):
            TR.one_euro_track(track, **bad)
    assert launches == []


def test_a_cpu_tensor_is_refused():
    tr = R.make_track(1, 9, 4, 13)
    with pytest.raises(L.RiggsHipError):
        TR.smooth_track(_dict(tr, 0), 1.0)
    with pytest.raises(L.RiggsHipError):
        TR.one_euro_track(_dict(tr, 0), 30.0)
