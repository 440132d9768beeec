"""CPU: the float64 restatement of the optical-flow term (tests/flow_ref.py) against the fixtures recorded from the reference's
own render_flow (tests/golden/make_flow_golden.py), its loss against finite differences and against the reference's inline
statements, ``landmark_interpolate`` against recorded values, and the planted faults against the bounds the GPU tests use."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from tests import flow_ref as FR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN, "flow_*.npz")) if "loss_ref" not in p)


def test_every_case_of_the_issue_has_a_fixture():
    assert set(CASES) >= {"mask_aniso", "nomask_iso", "one_camera", "float_rotation", "scale_const", "quat_product", "cov_python",
                          "principal_point_K"}


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_fixture(case):
    z = FR.load_fixture(os.path.join(GOLDEN, "flow_%s.npz" % case))
    logit = z["feature"][:, -1] if z["with_motion_mask"] else None
    F1, F2 = z["proj1"], z["proj2"]
    if not z["has_camera2"]:
        assert torch.equal(F1, F2)
    # the settings render_flow builds
    assert z["shs_is_none"] and z["sh_degree"] == 0 and torch.equal(z["bg"], torch.zeros(3))
    assert torch.equal(z["projmatrix"], F1) and torch.equal(z["viewmatrix"], z["view1"]) and torch.equal(z["campos"], z["campos1"])
    assert (z["image_height"], z["image_width"]) == (z["H"], z["W"])
    assert z["tanfovx"] == np.tan(z["fovx"] * 0.5) and z["tanfovy"] == np.tan(z["fovy"] * 0.5)
    # colours: the reference's float32 result within the derived bound (+ its own recorded error) of the float64 restatement
    r, units = FR.colour_ratio(z["colors_precomp"], z["xyz"], z["d_xyz1"], z["d_xyz2"], F1, F2, logit, extra=z["colour_ref_err"])
    assert r <= 1.0, (r, units)
    # ... and the restatement in float32 (the torch-op form) equals it to rounding
    m32 = None if logit is None else torch.sigmoid(logit[:, None])
    c32 = FR.colours(z["xyz"], z["d_xyz1"], z["d_xyz2"], F1, F2 if z["has_camera2"] else None, m32)
    assert FR.colour_ratio(c32, z["xyz"], z["d_xyz1"], z["d_xyz2"], F1, F2, logit)[0] <= 1.0
    assert float((c32 - z["colors_precomp"]).abs().max()) <= 2 * z["colour_ref_err"]
    # the glue tensors
    glue = FR.render_flow_glue(z["xyz"], z["scaling"], z["rotation"], z["opacity"], bool(z["isotropic"]), **FR.fixture_glue_args(z))
    for k in ("means3D", "opacities", "scales", "rotations", "cov3D_precomp"):
        if glue[k] is None:
            assert z[k].numel() == 0, k
        else:
            torch.testing.assert_close(glue[k], z[k].reshape(glue[k].shape), rtol=2e-6, atol=1e-7, msg=k)
    # gradients of the seeded cotangent
    got = (z["grad_d_xyz1"], z["grad_d_xyz2"], z["grad_feature"][:, -1] if logit is not None else None)
    ratios = FR.colour_grad_ratios(got, z["cotangent"], z["xyz"], z["d_xyz1"], z["d_xyz2"], F1, F2, logit,
                                   extra=tuple(float(e) for e in z["grad_ref_err"]))
    assert max(ratios) <= 1.0, ratios
    if logit is not None:
        assert float(z["grad_feature"][:, :-1].abs().max()) == 0.0


def test_landmark_interpolate_matches_recorded_reference_values():
    from riggs_amd.loss import landmark_interpolate
    z = json.load(open(os.path.join(GOLDEN, "flow_landmarks.json")))
    assert z["steps"] == [0, 15000, 25000, 25001] and 0 in z["at"] and 25001 in z["at"]
    for mode in ("log", "linear"):
        got = [float(landmark_interpolate(z["landmarks"], z["steps"], s, interpolation=mode)) for s in z["at"]]
        assert got == z[mode], mode
    assert landmark_interpolate(z["landmarks"], z["steps"], 25001) == 0 and landmark_interpolate(z["landmarks"], z["steps"], -1) == 0
    with pytest.raises(NotImplementedError):
        landmark_interpolate(z["landmarks"], z["steps"], 100, interpolation="cubic")


def _loss_inputs(seed, C, H, W, MC, dead=False):
    g = torch.Generator().manual_seed(seed)
    image, gt = torch.rand(C, H, W, generator=g), torch.rand(C, H, W, generator=g)
    motion = 0.2 * torch.randn(3, H, W, generator=g)
    alpha = torch.rand(1, H, W, generator=g) * 0.6 + 0.45        # straddles 0.5 and 0.9
    flow = 8.0 * torch.randn(H, W, 2, generator=g)
    masks = (torch.rand(H, W, MC, generator=g) > 0.45).float()
    if dead:
        masks[..., :2] = 0.0
    return image, gt, motion, alpha, flow, masks, 0.30, 0.55


def test_loss_restatement_matches_the_reference_statements():
    """flow_loss_ref.npz holds what train_gui.py:1101-1120 computed, executed as they stand in the reference."""
    z = FR.load_fixture(os.path.join(GOLDEN, "flow_loss_ref.npz"))
    args = (z["image"], z["gt"], z["motion"], z["alpha"], z["flow"], z["masks"], z["fid1"], z["fid2"])
    w32 = FR.flow_weight(z["image"], z["gt"], z["alpha"], z["masks"], z["fid1"], z["fid2"])[0]
    torch.testing.assert_close(w32, z["weight"], rtol=1e-6, atol=1e-7)
    r_loss, r_grad, share = FR.loss_ratios(torch.tensor(z["loss"]), z["grad_motion"], *args)
    assert r_loss <= 1.0 and r_grad <= 1.0 and share == 0.0, (r_loss, r_grad, share)


def test_loss_gradient_against_finite_differences():
    image, gt, motion, alpha, flow, masks, f1, f2 = _loss_inputs(3, 3, 9, 13, 2)
    loss, grad, _, _, und, live = FR.flow_loss_parts(image, gt, motion, alpha, flow, masks, f1, f2)
    assert int(und.sum()) == 0 and 0 < int(live.sum()) < live.numel()
    d = lambda t: t.double()  # noqa: E731
    f = lambda m: FR.flow_loss(d(image), d(gt), m, d(alpha), d(flow), d(masks), f1, f2)  # noqa: E731
    m0, h = motion.double(), 1e-6
    H, W = motion.shape[1:]
    c = flow.double() / torch.tensor([W, H], dtype=torch.float64) * 2
    away = ((c - m0[:2].permute(1, 2, 0)).abs() > 1e-3).permute(2, 0, 1)  # (away from the kink of | . |)
    checked = 0
    for k in range(3):
        for y in range(H):
            for x in range(W):
                if k < 2 and not bool(away[k, y, x]):
                    continue
                e = torch.zeros_like(m0)
                e[k, y, x] = h
                fd = float(f(m0 + e) - f(m0 - e)) / (2 * h)
                assert abs(fd - float(grad[k, y, x])) <= 1e-9, (k, y, x)
                checked += 1
    assert checked > 300
    assert float(grad[2].abs().max()) == 0.0 and float(grad[:2][:, ~live].abs().max()) == 0.0


@pytest.mark.parametrize("H,W,MC", [(1, 1, 2), (17, 33, 3), (800, 800, 4)])
def test_continuous_inputs_leave_no_undecidable_signs(H, W, MC):
    """The GPU tests' inputs: continuous random motion and flow — the restatement alone excludes none or a handful."""
    args = _loss_inputs(100 + H, 3, H, W, MC)
    _, _, _, _, und, live = FR.flow_loss_parts(*args)
    assert int(und.any(-1).sum()) <= max(3, 1e-5 * int(live.sum()))


def test_all_dead_mask_is_exactly_zero():
    args = _loss_inputs(7, 3, 17, 33, 3, dead=True)
    loss, grad, lb, _, _, live = FR.flow_loss_parts(*args)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0 and lb == 0.0 and not bool(live.any())


# ---- planted faults: each is rejected by the bound the GPU tests apply to the kernels -------------------------------------
def test_planted_fault_swapped_projection_is_rejected():
    z = FR.load_fixture(os.path.join(GOLDEN, "flow_mask_aniso.npz"))
    args = (z["xyz"], z["d_xyz1"], z["d_xyz2"], z["proj1"], z["proj2"])
    m = torch.sigmoid(z["feature"][:, -1:])
    assert FR.colour_ratio(FR.colours(*args, m), *args, z["feature"][:, -1])[0] <= 1.0
    assert FR.colour_ratio(FR.colours(*args, m, fault="swap_F2"), *args, z["feature"][:, -1])[0] > 1e3


def test_planted_fault_w_plus_1e_minus_7_is_rejected():
    args = FR.near_plane_case(300, 5)
    hw = torch.cat([args[0] + args[1], torch.ones(300, 1)], -1) @ args[3]
    assert 0.01 <= float(hw[:, 3].min()) and float(hw[:, 3].max()) <= 0.11
    assert FR.colour_ratio(FR.colours(*args, None), *args)[0] <= 1.0
    assert FR.colour_ratio(FR.colours(*args, None, fault="w_eps"), *args)[0] > 1.0
    g = torch.randn(300, 3, generator=torch.Generator().manual_seed(6))
    grads = lambda fault: torch.autograd.grad(  # noqa: E731
        (FR.colours(args[0], a1, a2, args[3], args[4], None, fault=fault) * g).sum(), [a1, a2])
    a1, a2 = args[1].clone().requires_grad_(True), args[2].clone().requires_grad_(True)
    assert max(FR.colour_grad_ratios(tuple(grads(None)) + (None,), g, *args)) <= 1.0
    assert max(FR.colour_grad_ratios(tuple(grads("w_eps")) + (None,), g, *args)) > 1.0


def test_planted_fault_normalise_after_add_is_rejected():
    z = FR.load_fixture(os.path.join(GOLDEN, "flow_mask_aniso.npz"))
    bad = FR.render_flow_glue(z["xyz"], z["scaling"], z["rotation"], z["opacity"], False, fault="normalise_after_add",
                              **FR.fixture_glue_args(z))
    with pytest.raises(AssertionError):
        torch.testing.assert_close(bad["rotations"], z["rotations"], rtol=2e-6, atol=1e-7)
    assert float((bad["rotations"] - z["rotations"]).abs().max()) > 1e-2


def test_planted_fault_alpha_threshold_is_rejected():
    args = _loss_inputs(11, 3, 17, 33, 3)
    d = lambda t: t.double() if isinstance(t, torch.Tensor) else t  # noqa: E731
    m = args[2].double().requires_grad_(True)
    dd = list(map(d, args))
    bad = FR.flow_loss(dd[0], dd[1], m, *dd[3:], fault="alpha_half")
    gbad, = torch.autograd.grad(bad, m)
    r_loss, r_grad, _ = FR.loss_ratios(bad.detach(), gbad, *args)
    assert r_loss > 1e3 and r_grad > 1e3
    good = FR.flow_loss(dd[0], dd[1], m, *dd[3:])
    ggood, = torch.autograd.grad(good, m)
    r = FR.loss_ratios(good.detach().float(), ggood.float(), *args)
    assert r[0] <= 1.0 and r[1] <= 1.0
