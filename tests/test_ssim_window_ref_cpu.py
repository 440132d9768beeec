"""The references of tests/ssim_window_ref.py on the host: the per-pixel bounds accept the numpy float32 restatement of the image
loss and of the evaluation report on every case of the GPU grid, with the epilogues fused and unfused, and reject each planted
fault on the arrays it spoils and on no others; the vacuity cap and the denominator condition hold on every scored case; the
two float64 references of the loss agree; the trainer's window is one rounding per tap from the exact product; the restated
``metrics_plan`` agrees with the C ABI's host-side size query."""
import numpy as np
import pytest

from tests import ssim_window_ref as S

GRID = S.grid()
_BY_NAME = {c["name"]: c for c in GRID}
OPTION_SHAPES = (((3, 65, 33), "noisy"), ((1, 11, 38), "dark"))


def test_grid_covers_the_sizes_the_families_and_the_options():
    assert len(_BY_NAME) == len(GRID)
    shapes = {c["shape"] for c in GRID}
    assert {s[2] for s in shapes} >= set(S.WS) | {70} and {s[1] for s in shapes} >= set(S.HS) | {130}
    assert {s[0] for s in shapes} == set(S.CS) | {2} and {(2, 130, 70), (3, 65, 33), (4, 16, 16)} <= shapes
    for W in S.WS:
        assert all(any(s[1:] == (H, W) for s in shapes) for H in (1, 11, 65))
    for H in S.HS:
        assert all(any(s[1:] == (H, W) for s in shapes) for W in (1, 11, 33))
    for fam in S.FAMILIES:
        assert len({c["shape"] for c in GRID if c["family"] == fam}) >= 3, fam
    for shape in shapes:
        assert len({c["family"] for c in GRID if c["shape"] == shape}) == 2
    assert {c["lam"] for c in GRID} == set(S.LAMBDAS) and {c["g"] for c in GRID} >= set(S.G_OPTIONS[4:])


def test_the_trainers_window_is_one_rounding_per_tap_from_the_exact_product():
    from oracle import loss_ref as O
    assert S.window_distance() <= 1.0
    w = S.win_f32()
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 11 * S.U
    # the serial float32 sum of fill_window_f32 against numpy's pairwise one (the oracle's): one rounding of the sum at the most
    assert np.abs(w.astype(np.float64) - O.window1d()).max() <= 2 * S.U * w.max()
    assert np.abs(S.win_f64().astype(np.float64) - w).max() <= 2 * S.U * w.max()


@pytest.mark.parametrize("shape,family", [((3, 65, 33), "noisy"), ((1, 11, 38), "uniform"), ((2, 130, 70), "dark")])
def test_the_two_float64_references_agree(shape, family):
    """oracle/loss_ref.py (the trainer's rounded 2-D window, a direct 121-tap sum) against the separable exact-product form."""
    from oracle import loss_ref as O
    x, y = S.make_images(shape, family)
    ref = S.loss_reference(x, y)
    X, Y = x.astype(np.float64), y.astype(np.float64)
    _, *mo = O._moments(X, Y)
    for a, b, mag in zip(ref["moments"], mo, (np.abs(X), np.abs(Y), X * X, Y * Y, np.abs(X * Y))):
        scale = S.conv64(mag, S.win_f32())
        assert (np.abs(a - b) <= 1e-6 * scale).all()
    assert abs(ref["ssim"].v.mean() - O.ssim(x, y)) <= 2e-6
    gl, gs = S.effective_g((0.7, -0.3, None), 0.2)
    dx = S.dx_reference(x, y, [ref[k] for k in ("dmu", "de11", "de12")], 0.2, (0.7, -0.3, None))
    want = O.grad(x, y, float(gl.v), float(gs.v))
    assert np.abs(dx.v - want).max() <= 2e-5 * np.abs(want).max()


@pytest.mark.parametrize("case", GRID, ids=[c["name"] for c in GRID])
def test_restatement_is_accepted_and_the_inputs_are_not_vacuous(case):
    """Also the denominator condition (S.Denominator is raised by the reference where a divisor's bound reaches half of it) and, on
    the structural families, bound <= 2 n u x (the expression in absolute values)."""
    for fused in (False, True):
        x, y, state, out3, dx = S.restate_case(case, fused=fused)
        res = S.check_loss(case, x, y, state, out3, dx)
        assert not S.bad_arrays(res), (fused, {k: res[k] for k in S.bad_arrays(res)})
        assert res["nan_free"]
        assert not S.vacuous_arrays(res), S.vacuous_arrays(res)
        if case["family"] in S.STRUCTURAL:
            assert 0.0 < res["structural"] <= 1.0
        if case["family"] == "identical":   # the reference is 0: |dx| <= its bound
            assert res["dx_zero"]["bad"] == 0 and res["dx_zero"]["n"] == x.size


@pytest.mark.parametrize("shape,family", OPTION_SHAPES)
def test_backward_options(shape, family):
    case = {"name": "options", "shape": shape, "family": family, "lam": 0.2, "g": S.G_OPTIONS[7]}
    x, y = S.make_images(shape, family)
    state, out3 = S.restate_loss_forward(x, y, 0.2)
    ref = S.loss_reference(x, y)
    for g in S.G_OPTIONS:
        for lam in S.LAMBDAS:
            dx = S.restate_loss_backward(x, y, state, lam, g)
            res = S.check_loss(dict(case, lam=lam), x, y, state, S.restate_loss_forward(x, y, lam)[1], dx, g=g, ref=ref)
            assert not S.bad_arrays(res), (g, lam, S.bad_arrays(res))
            if g == S.G_OPTIONS[0]:
                assert not dx.any()
    for lam in S.LAMBDAS:   # the g_loss route against the g_l1 / g_ssim route with the same effective coefficients
        a = S.restate_loss_backward(x, y, state, lam, (None, None, 1.3))
        b = S.restate_loss_backward(x, y, state, lam, S.split_route(lam, 1.3))
        assert S.routes_agree(x, y, state, lam, 1.3, a, b)
    same = S.restate_loss_backward(x, x.copy(), state, 0.2, (0.7, None, None))
    assert not same.any()


@pytest.mark.parametrize("fault", sorted(S.LOSS_FAULTS))
def test_planted_loss_fault_is_rejected_on_the_arrays_it_spoils(fault):
    case, spoils = S.fault_case(fault)
    x, y, state, out3, dx = S.restate_case(case)
    assert not S.bad_arrays(S.check_loss(case, x, y, state, out3, dx))
    x, y, state, out3, dx = S.restate_case(case, fault=fault)
    assert set(S.bad_arrays(S.check_loss(case, x, y, state, out3, dx))) == spoils


def test_the_other_window_is_not_seen():
    """fill_window_f64 in place of fill_window_f32 is one rounding per tap: inside the 22 u of the window bound, as expected."""
    case, _ = S.fault_case("h_tap_0")
    x, y, state, out3, dx = S.restate_case(case, win=S.win_f64())
    res = S.check_loss(case, x, y, state, out3, dx)
    assert not S.bad_arrays(res)
    clean = S.check_loss(case, *S.restate_case(case))
    assert max(res[k]["worst"] for k in ("dmu", "de11", "de12")) <= 1.0 and clean["dmu"]["worst"] > 0.0


@pytest.mark.parametrize("name,shape,family,ms", S.METRICS_CASES, ids=[c[0] for c in S.METRICS_CASES])
def test_metrics_restatement_is_accepted(name, shape, family, ms):
    x, y = S.metrics_inputs(shape, family)
    for fused in (False, True):
        got = S.restate_metrics(x, y, False, ms, fused=fused)
        res = S.check_metrics(x, y, False, ms, got)
        assert not S.bad_arrays(res), {k: res[k] for k in S.bad_arrays(res)}
        assert not S.vacuous_arrays(res)


@pytest.mark.parametrize("fault", sorted(S.METRICS_FAULTS))
def test_planted_metrics_fault_is_rejected_on_the_arrays_it_spoils(fault):
    name, spoils = S.METRICS_FAULTS[fault]
    _, shape, family, ms = next(c for c in S.METRICS_CASES if c[0] == name)
    x, y = S.metrics_inputs(shape, family)
    got = S.restate_metrics(x, y, False, ms, fault=fault)
    assert set(S.bad_arrays(S.check_metrics(x, y, False, ms, got))) == spoils


def test_clamp_on_load_is_the_clamped_input_in_the_restatement():
    x, y = S.metrics_inputs((1, 75, 43), "noisy")
    x, y = np.float32(x * 1.4 - 0.2), np.float32(y * 1.4 - 0.2)
    a = S.restate_metrics(x, y, True, False)
    b = S.restate_metrics(np.clip(x, 0, 1), np.clip(y, 0, 1), False, False)
    assert np.array_equal(a["partial"], b["partial"]) and x.min() < 0 and x.max() > 1
    assert not S.bad_arrays(S.check_metrics(x, y, True, False, a))


def test_restated_plan_agrees_with_the_size_query():
    """riggs_image_metrics_workspace_floats is host code: no GPU is touched."""
    from riggs_amd import _lib
    L = _lib.lib()
    shapes = [(1,) + c[1] for c in S.METRICS_CASES] + [(2, 3, 200, 200), (1, 3, 160, 160), (3, 1, 161, 640), (1, 3, 800, 800), (2, 1, 640, 641),
                                                       (1, 1, 896, 900), (1, 2, 384, 384), (1, 1, 10, 300), (5, 4, 383, 1000)]
    for B, C, H, W in shapes:
        p = S.plan(B, C, H, W)
        assert p["total_floats"] == L.riggs_image_metrics_workspace_floats(B, C, H, W), (B, C, H, W)
        assert p["img"][1] in (0, 2 * p["doubles"]) and p["part"][0] == 0
    assert S.plan(1, 1, 640, 640)["f"] == 2 and S.plan(1, 1, 896, 896)["f"] == 4 and S.plan(1, 1, 385, 385)["f"] == 2
    assert S.state_floats(2, 130, 70) == L.riggs_l1_ssim_state_floats(2, 130, 70) == 3 * 2 * 130 * 70 + 2 * 18
