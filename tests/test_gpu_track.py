"""-m gpu: riggs_amd.track (csrc/track.hip) against tests/track_ref.py — float64 (eigh) is the oracle, its float32 form (the
kernel's order of sums and its Jacobi sweeps, every operation rounded) the yardstick for rounding.

Bars.  PARITY per case and tensor: max(8 * e32, 1e-6), e32 = the float32 restatement's own deviation from float64 on that case;
rotations by the angle between the two rotations (2 acos |dot|, rad), translations relative to the track's extent.  The margin and
the floor are those of tests/test_gpu_ik.py, for its reason: the hardware's sqrt and division, for the one-euro filter also acos
and sin.  ``support`` 1e-6 of the case's largest, unit norms 1e-6.  The exact properties are bit equalities.  With
RIGGS_TRACK_PARITY_JSON set to a path, what was measured is written there (profiles/track_parity.json is such a record).

Shapes (tests/track_ref.py: CASES): T in {1, 2, R, R + 1, 2R + 1, 2R + 2} for R in {0, 1, 6, 64} (the clipped window, the whole
track inside one window, wrap from the smallest T it accepts), B T J in {1, 255, 256, 257, 3 * 256 + 5} (the last lane of a block,
the first of the next, several blocks), J in {1, 24, 65, 256}, B in {1, 3}, wrap both ways."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from riggs_amd import _lib as L  # noqa: E402
from riggs_amd import track as TR  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import track_ref as R  # noqa: E402
from tests.pose_solve_util import T, bits, parity_report  # noqa: E402

_REPORT, _GPU = {}, {}
report = parity_report("RIGGS_TRACK_PARITY_JSON", _REPORT)
BY_NAME = {c["name"]: c for c in R.CASES}


def npy(out, keys):
    return {k: out[k].cpu().numpy() for k in keys}


def as_track(tr, B):
    """The generator's arrays as smooth_track / one_euro_track take them: with the batch axis for B > 1, without it for B = 1."""
    pick = (lambda a: T(a)) if B > 1 else (lambda a: T(a[0]))
    return {"local_rotation": pick(tr["rot"]), "global_trans": pick(tr["trans"])}, pick(tr["weights"]), pick(tr["trans_weights"])


def smooth_gpu(case, tr):
    track, w, tw = as_track(tr, case["B"])
    out = TR.smooth_track(track, case["sigma"], radius=case["R"], weights=w, trans_weights=tw, wrap=case["wrap"])
    assert out["local_rotation"] is out["local_rotation2"] and out["num"] == case["T"]
    o, (B, Tn, J) = npy(out, ("local_rotation", "global_trans", "support")), (case["B"], case["T"], case["J"])
    return {"local_rotation": o["local_rotation"].reshape(B, Tn, J, 4), "global_trans": o["global_trans"].reshape(B, Tn, 3),
            "support": o["support"].reshape(B, Tn, J)}


def case_gpu(case):
    """The kernel's result on a case: computed once, shared, never changed."""
    if case["name"] not in _GPU:
        _GPU[case["name"]] = smooth_gpu(case, R.case_reference(case)[0])
    return _GPU[case["name"]]


def measure(got, o64, o32, extent):
    """(deviation of the kernel from float64, e32, bar) per tensor."""
    dev = {"local_rotation": float(R.rotation_angle(got["local_rotation"], o64["local_rotation"]).max()),
           "global_trans": float(np.abs(got["global_trans"].astype(np.float64) - o64["global_trans"]).max() / extent)}
    e32 = {"local_rotation": float(R.rotation_angle(o32["local_rotation"], o64["local_rotation"]).max()),
           "global_trans": float(np.abs(o32["global_trans"].astype(np.float64) - o64["global_trans"]).max() / extent)}
    return dev, e32, {k: max(8 * e32[k], 1e-6) for k in e32}


def unit_norms(q, what):
    err = float(np.abs(np.linalg.norm(q.astype(np.float64), axis=-1) - 1).max())
    assert err <= 1e-6, "%s: |q| off by %.3g" % (what, err)


# ------------------------------------------------------------------------------------------------ the Gaussian window
@pytest.mark.parametrize("name", list(BY_NAME))
def test_smooth_parity_with_the_float64_oracle(name):
    case = BY_NAME[name]
    tr, o64, o32 = R.case_reference(case)
    got = case_gpu(case)
    assert got["local_rotation"].shape == o64["local_rotation"].shape and np.isfinite(got["local_rotation"]).all()
    dev, e32, bar = measure(got, o64, o32, R.trans_extent(tr["trans"]))
    sup = float(np.abs(got["support"].astype(np.float64) - o64["support"]).max() / max(o64["support"].max(), 1e-12))
    _REPORT["smooth-" + name] = {"e32": e32, "gpu": dev, "bar": bar, "support": sup,
                                 "bits_differing_from_float32": int((bits(got["local_rotation"]) != bits(o32["local_rotation"])).sum())}
    print(name, "e32", e32, "gpu", dev, "support", sup)
    failed = ["%s: %.3g > %.3g (e32 %.3g)" % (k, dev[k], bar[k], e32[k]) for k in dev if not dev[k] <= bar[k]]
    assert not failed, "; ".join(failed)
    assert sup <= 1e-6, sup
    unit_norms(got["local_rotation"], name)
    # no support exactly where the oracle has none; there the normalised input or the identity, and the input translation
    none = o64["support"] == 0
    assert np.array_equal(got["support"] == 0, none)
    assert np.array_equal(bits(got["local_rotation"][none]), bits(o32["local_rotation"][none]))
    # the sign: the centre sample's hemisphere where it is valid, else the first non-zero component positive
    q32, qok = R.unit(tr["rot"], np.float32)
    valid = qok & (tr["weights"] > 0)
    assert (R.dot4(got["local_rotation"], q32)[valid] >= 0).all()
    lead = got["local_rotation"][~valid & ~none]
    first = np.take_along_axis(lead, np.argmax(lead != 0, -1)[:, None], -1)
    assert (first > 0).all()


def test_radius_zero_returns_the_normalised_input():
    case = BY_NAME["b1_t2_j24_r0"]
    tr, _, o32 = R.case_reference(case)
    got = case_gpu(case)
    q32, qok = R.unit(tr["rot"], np.float32)
    # (M = c q q^T with two roundings per entry: 2^-23 of its one eigenvalue, over a gap of that eigenvalue; as many again for the sweeps)
    assert float(R.rotation_angle(got["local_rotation"], q32.astype(np.float64)).max()) <= 4e-6
    gap = ~(tr["weights"] > 0)
    assert gap.any() and np.array_equal(bits(got["local_rotation"][gap]), bits(q32[gap])) and (got["support"][gap] == 0).all()
    assert np.array_equal(bits(got["support"][~gap]), bits(tr["weights"][~gap]))


def _one(name="b1_t14_j24_r6"):
    case = BY_NAME[name]
    tr = R.case_reference(case)[0]
    return case, {k: v.copy() for k, v in tr.items()}


def _same(a, b, keys=("local_rotation", "global_trans", "support")):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


@pytest.mark.parametrize("name", ["b1_t14_j24_r6", "b1_t14_j24_r6_wrap", "b3_t14_j65_r6"])
def test_a_sample_sign_changes_no_bit_but_the_centre_negates_its_output(name):
    case, tr = _one(name)
    base = case_gpu(case)
    valid = R.unit(tr["rot"], np.float32)[1] & (tr["weights"] > 0)
    b, t, j = (int(v[0]) for v in np.nonzero(valid & (base["support"] > 0)))
    tr["rot"][b, t, j] *= -1
    got = smooth_gpu(case, tr)
    want = base["local_rotation"].copy()
    want[b, t, j] *= -1  # only the frame whose CENTRE sample this is: every other window does not see the sign
    assert np.array_equal(bits(got["local_rotation"]), bits(want))
    assert _same(got, base, ("global_trans", "support"))
    assert (R.dot4(got["local_rotation"], tr["rot"])[valid] >= 0).all()


def test_a_nan_in_a_gap_changes_no_bit():
    case, tr = _one("b3_t14_j24_r6")
    base = case_gpu(case)
    # gaps by their confidence, where the sample's own window has support (without support the output IS the input sample)
    gap = ~(tr["weights"] > 0) & (base["support"] > 0)
    tgap = ~(tr["trans_weights"] > 0)
    assert gap.sum() > 50 and tgap.sum() > 3
    tr["rot"][gap] = np.nan
    tr["trans"][tgap] = np.nan
    assert _same(smooth_gpu(case, tr), base)
    # gaps by their values under a good confidence (NaN, zero, infinite): the same samples switched off by their weight
    on = np.argwhere(tr["weights"] > 0)[::17]
    off = {k: v.copy() for k, v in tr.items()}
    for n, (b, t, j) in enumerate(on):
        tr["rot"][b, t, j] = (np.nan, 0.0, np.inf)[n % 3]
    off["weights"][tuple(on.T)] = 0
    got, ref = smooth_gpu(case, tr), smooth_gpu(case, off)
    held = ref["support"] > 0  # (without support: the identity here, the normalised input there)
    assert held.mean() > 0.9 and np.array_equal(bits(got["local_rotation"][held]), bits(ref["local_rotation"][held]))
    assert _same(got, ref, ("global_trans", "support")) and np.isfinite(got["local_rotation"]).all() and np.isfinite(got["global_trans"]).all()


@pytest.mark.parametrize("name", ["b3_t14_j24_r6", "b3_t14_j24_r6_wrap", "b3_t85_j1_r6", "b3_t3_j256_r1"])
def test_runs_are_bit_identical_and_tracks_independent(name):
    case = BY_NAME[name]
    tr = R.case_reference(case)[0]
    base = case_gpu(case)
    assert _same(smooth_gpu(case, tr), base)
    for b in range(case["B"]):
        alone = smooth_gpu(dict(case, B=1), {k: v[b:b + 1] for k, v in tr.items()})
        assert all(np.array_equal(bits(alone[k][0]), bits(base[k][b])) for k in alone), b


def test_one_translation_for_the_track_passes_through():
    case, tr = _one()
    const = torch.randn(1, 3, device="cuda")
    out = TR.smooth_track({"local_rotation2": T(tr["rot"][0]), "global_trans": const, "d_nodes": const, "residual": const}, case["sigma"],
                          radius=case["R"], weights=T(tr["weights"][0]))
    assert out["global_trans"] is const and sorted(out) == ["global_trans", "local_rotation", "local_rotation2", "num", "support"]
    assert np.array_equal(bits(out["local_rotation"].cpu().numpy()), bits(case_gpu(case)["local_rotation"][0]))
    # (T, 1, 3) translations are (T, 3) translations
    out = TR.smooth_track({"local_rotation": T(tr["rot"][0]), "global_trans": T(tr["trans"][0])[:, None]}, case["sigma"], radius=case["R"],
                          weights=T(tr["weights"][0]), trans_weights=T(tr["trans_weights"][0]))
    assert np.array_equal(bits(out["global_trans"].cpu().numpy()), bits(case_gpu(case)["global_trans"][0]))


# ------------------------------------------------------------------------------------------------ the one-euro filter
def euro_gpu(tr, B, sl=slice(None), state=None):
    cut = {k: v[:, sl] for k, v in tr.items()}
    track, w, tw = as_track(cut, B)
    out = TR.one_euro_track(track, weights=w, trans_weights=tw, state=state, **R.EURO)
    Tn = cut["rot"].shape[1]
    return out["local_rotation"].cpu().numpy().reshape(B, Tn, -1, 4), out["global_trans"].cpu().numpy().reshape(B, Tn, 3), out["state"]


@pytest.mark.parametrize("J,B", [(24, 1), (256, 1), (24, 3)])
def test_one_euro_parity_with_the_float64_oracle(J, B):
    tr = R.euro_track(B, J, 300 + J + B)
    assert (tr["weights"][:, 0] == 0).all() and (tr["weights"][:, 20:25] == 0).all() and (tr["weights"][:, -1] == 0).all()
    kw = dict(weights=tr["weights"], trans_weights=tr["trans_weights"], **R.EURO)
    o64 = R.one_euro(tr["rot"], tr["trans"], dtype=np.float64, **kw)
    o32 = R.one_euro(tr["rot"], tr["trans"], dtype=np.float32, **kw)
    rot, trans, state = euro_gpu(tr, B)
    dev, e32, bar = measure({"local_rotation": rot, "global_trans": trans}, o64, o32, R.trans_extent(tr["trans"]))
    _REPORT["one_euro-j%d-b%d" % (J, B)] = {"e32": e32, "gpu": dev, "bar": bar}
    print(J, B, "e32", e32, "gpu", dev)
    failed = ["%s: %.3g > %.3g (e32 %.3g)" % (k, dev[k], bar[k], e32[k]) for k in dev if not dev[k] <= bar[k]]
    assert not failed, "; ".join(failed)
    unit_norms(rot, "one-euro")
    assert (rot[:, 0] == np.array([1, 0, 0, 0], np.float32)).all() and (trans[:, 0] == 0).all()  # before any sample
    assert np.array_equal(bits(rot[:, 20:25]), bits(np.repeat(rot[:, 19:20], 5, 1)))  # a gap frame holds
    assert np.array_equal(state["gap"].cpu().numpy(), o64["state"]["gap"]) and (state["gap"].cpu().numpy() >= 1).all()
    assert np.array_equal(state["trans_gap"].cpu().numpy(), o64["state"]["trans_gap"])
    assert float(R.rotation_angle(state["rotation"].cpu().numpy(), rot[:, -1]).max()) == 0.0


@pytest.mark.parametrize("T1", [1, 17])
def test_one_euro_in_two_calls_and_frame_by_frame_gives_the_same_bits(T1):
    B, J = 1, 24
    tr = R.euro_track(B, J, 311)
    rot, trans, state = euro_gpu(tr, B)
    r1, t1, s1 = euro_gpu(tr, B, slice(0, T1))
    kept = {k: v.clone() for k, v in s1.items()}
    r2, t2, s2 = euro_gpu(tr, B, slice(T1, None), state=s1)
    assert np.array_equal(bits(np.concatenate([r1, r2], 1)), bits(rot)) and np.array_equal(bits(np.concatenate([t1, t2], 1)), bits(trans))
    assert all(torch.equal(s2[k], state[k]) for k in state) and all(torch.equal(kept[k], s1[k]) for k in kept)
    # OneEuroTrack: the same code one frame per launch, its state updated in place
    f = TR.OneEuroTrack(J, **R.EURO)
    held = {k: v.data_ptr() for k, v in f.state.items()}
    for rep in range(2):
        got = [f.filter({"local_rotation": T(tr["rot"][0, t]), "global_trans": T(tr["trans"][0, t:t + 1])}, weights=T(tr["weights"][0, t]),
                        trans_weight=T(tr["trans_weights"][0, t:t + 1])) for t in range(tr["rot"].shape[1])]
        assert np.array_equal(bits(torch.stack([g["local_rotation"] for g in got]).cpu().numpy()), bits(rot[0])), rep
        assert np.array_equal(bits(torch.cat([g["global_trans"] for g in got]).cpu().numpy()), bits(trans[0])), rep
        assert all(torch.equal(f.state[k], state[k]) for k in state) and held == {k: v.data_ptr() for k, v in f.state.items()}
        f.reset()


def test_one_euro_tracks_are_independent():
    tr = R.euro_track(3, 24, 314)
    rot, trans, _ = euro_gpu(tr, 3)
    for b in range(3):
        r, t, _ = euro_gpu({k: v[b:b + 1] for k, v in tr.items()}, 1)
        assert np.array_equal(bits(r[0]), bits(rot[b])) and np.array_equal(bits(t[0]), bits(trans[b]))


# ------------------------------------------------------------------------------------------------ capture, downstream, refusals
def _capture(step):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    return graph, out


def test_smooth_track_is_captured_and_replayed():
    case, tr = _one()
    rot, trans, w, tw = T(tr["rot"][0]), T(tr["trans"][0]), T(tr["weights"][0]), T(tr["trans_weights"][0])

    def step():
        return TR.smooth_track({"local_rotation": rot, "global_trans": trans}, case["sigma"], radius=case["R"], weights=w, trans_weights=tw)
    graph, out = _capture(step)
    g = torch.Generator().manual_seed(3)
    for rep in range(2):
        rot.add_(0.1 * torch.randn(rot.shape, generator=g).cuda())
        trans.add_(0.1 * torch.randn(trans.shape, generator=g).cuda())
        w[rep + 2] = 0.0
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        assert all(torch.equal(eager[k], out[k]) for k in ("local_rotation", "global_trans", "support")), rep


def test_the_streaming_filter_is_captured_and_replayed():
    J = 24
    tr = R.euro_track(1, J, 317, T=12)
    pose = {"local_rotation": T(tr["rot"][0, 0]), "global_trans": T(tr["trans"][0, :1])}
    w, tw = T(tr["weights"][0, 0]), T(tr["trans_weights"][0, :1])
    f = TR.OneEuroTrack(J, **R.EURO)
    graph, out = _capture(lambda: f.filter(pose, weights=w, trans_weight=tw))
    f.reset()  # (the warm-up and the capture's own launch-free recording left the state as it was or advanced it: start over)
    ref = TR.OneEuroTrack(J, **R.EURO)
    for t in range(12):
        for dst, src in ((pose["local_rotation"], tr["rot"][0, t]), (pose["global_trans"], tr["trans"][0, t:t + 1]), (w, tr["weights"][0, t]),
                         (tw, tr["trans_weights"][0, t:t + 1])):
            dst.copy_(T(src))
        graph.replay()
        torch.cuda.synchronize()
        eager = ref.filter(pose, weights=w, trans_weight=tw)
        assert torch.equal(eager["local_rotation"], out["local_rotation"]) and torch.equal(eager["global_trans"], out["global_trans"]), t
    assert all(torch.equal(f.state[k], ref.state[k]) for k in f.state)


def test_the_smoothed_track_goes_through_the_rig():
    from riggs_amd import synth
    from riggs_amd.skeleton import SkeletonWarp
    from tests import playback_ref as P
    N, J, M = 257, 24, 14
    case = BY_NAME["b1_t14_j24_r6"]
    tr, o64, _ = R.case_reference(case)
    sc = synth.make_scene(N, J, 4321)
    sw = SkeletonWarp(joints=sc["joints"], parent_indices=sc["parents"], K=-1, hyper_dim=8, use_skinning_weight_mlp=False,
                      use_template_offsets=False).cuda()
    sw._node_radius.data = sc["node_radius"].clone().cuda()
    track, w, tw = as_track(tr, 1)
    smoothed = TR.smooth_track(dict(track, d_nodes=torch.zeros(M, J, 3, device="cuda")), case["sigma"], radius=case["R"], weights=w, trans_weights=tw)
    out = sw.deform_sequence(sc["xyz"].cuda(), smoothed, None)
    ref = P.deform_sequence(sc["xyz"], sc["joints"], sc["parents"], sc["node_radius"], torch.from_numpy(o64["local_rotation"][0]).float(),
                            torch.from_numpy(o64["global_trans"][0]).float(), torch.ones(N, 1), -1)
    assert out["d_nodes"].shape == (M, J, 3)
    U.assert_close(out["d_nodes"].cpu().numpy(), ref["d_nodes"].numpy(), "d_nodes of the smoothed track", 1e-5)


def test_refusals():
    case, tr = _one()
    track, w, tw = as_track(tr, 1)
    with pytest.raises(ValueError):
        TR.smooth_track(track, 2.0, radius=65)
    with pytest.raises(ValueError):
        TR.smooth_track(track, 2.0, radius=7, wrap=True)
    with pytest.raises(L.RiggsHipError):
        TR.smooth_track(track, 2.0, weights=w[:, :5])
    with pytest.raises(L.RiggsHipError):
        TR.smooth_track({k: v.cpu() for k, v in track.items()}, 2.0)
    with pytest.raises(L.RiggsHipError):
        TR.smooth_track({"local_rotation": torch.ones(2, 257, 4, device="cuda"), "global_trans": torch.zeros(2, 3, device="cuda")}, 1.0)
    # the C entries refuse the same on their own: nothing is launched (the outputs keep their fill)
    out, buf = U.out_buf((14 * 24, 4))
    z = torch.zeros(14 * 24 * 4, device="cuda")
    zi = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = z.data_ptr()
    for J, Rr, wrap in ((257, 1, 0), (24, 65, 0), (24, 7, 1), (0, 1, 0)):
        assert L.lib().riggs_track_smooth(1, 14, J, Rr, wrap, p, None, None, None, p, out.data_ptr(), None, p, L.stream_ptr()) != 0
        assert "riggs_track_smooth" in L.lib().riggs_last_error().decode()
    assert L.lib().riggs_track_smooth(1, 14, 24, 1, 0, p + 4, None, None, None, p, out.data_ptr(), None, p, L.stream_ptr()) != 0  # alignment
    for J, rate, fmin, beta in ((257, 30.0, 1.0, 0.0), (24, 0.0, 1.0, 0.0), (24, 30.0, 0.0, 0.0), (24, 30.0, 1.0, -1.0), (24, float("nan"), 1.0, 0.0)):
        assert L.lib().riggs_track_one_euro(1, 14, J, p, None, None, None, rate, fmin, beta, 1.0, 1.0, 0.0, p, p, zi.data_ptr(), None, None,
                                            None, out.data_ptr(), None, L.stream_ptr()) != 0
        assert "riggs_track_one_euro" in L.lib().riggs_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf == U.SENT).all())
