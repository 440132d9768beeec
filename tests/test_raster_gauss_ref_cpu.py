"""CPU: the float64 reference of the rasterizer's per-Gaussian stage (tests/raster_gauss_ref.py) and its bounds, checked on the host.

  * the reference's forward against the saved state of oracle/raster_ref.forward, element by element, within the bounds (the
    oracle is a float32 evaluation of the same steps); with the glue against the oracle's render_glue composition;
  * the reference's gradients composed with the float64 compositing of tests/dense_splat.py: the dense splat's own
    dL/d(per-Gaussian outputs) fed in as the record reproduce its end-to-end gradients to 1e-10;
  * a float32 restatement of the kernel's steps within every bound on every case of the GPU grid, in three evaluation orders;
  * planted faults, each rejected on the array it spoils; and the ones the old bars (gpu_util.assert_close as
    tests/test_gpu_raster.py calls it) let through;
  * the bounds are not vacuous on the GPU grid."""
import math

import numpy as np
import pytest
import torch

from oracle import deform_ref as O
from oracle import raster_ref as RR
from riggs_amd import synth
from tests import dense_splat as DS
from tests import gpu_util as GU
from tests import raster_gauss_ref as R
from tests import test_gpu_raster_gauss_f64 as G
from tests.test_oracle_raster import small_scene

GAUSS_CAP = 0.10  # the cap of tests/test_cnode_ref_cpu.py for per-Gaussian arrays
ALL = G.GRID + G.SPARSE_ZERO + [G.GUARD]
IDS = ["%d-%s" % (i, G.case_id(c)) for i, c in enumerate(ALL)]

_cache = {}


def prepared(c):
    """(tensors, records on the visible rows, {array: (reference, bound)}, forward reference, forward bounds) of a grid case."""
    key = G.case_id(c) + str(c["seed"])
    if key not in _cache:
        if len(_cache) > 4:
            _cache.pop(next(iter(_cache)))
        t = G.build(c)
        rec = G.mask_rows(t["rec"], t["vis"])
        ref = G.reference_of(c, t, rec, t["vis"], t["clamp_bits"])
        _cache[key] = (t, rec, ref, R.reference(t, c), R.bounds(t, c)[1])
    return _cache[key]


def restated(c, t, rec, order=0, fault=None):
    """The float32 restatement of the kernel's steps: {array: float32 tensor}, rows without a record exactly 0."""
    with torch.no_grad():
        o = R.kernel_steps(R.F32(order), t, c, rec=rec, clamp_bits=t["clamp_bits"], fault=fault)
    return R.collect(o, True, t["vis"] & (rec != 0).any(1))


def failing(got, ref):
    return sorted(k for k, (r, b) in ref.items() if R.violations(got[k].double().reshape(r.shape), r, b)[0])


# ----------------------------------------------------------------------------------------------- reference against the oracle
def scene_tensors(s, glue, raw=None):
    cam = s["cam"]
    t = {"view": cam.world_view_transform.contiguous(), "proj": cam.full_proj_transform.contiguous(), "campos": cam.camera_center.contiguous(),
         "tanx": float(np.float32(math.tan(cam.FoVx / 2))), "tany": float(np.float32(math.tan(cam.FoVy / 2)))}
    if glue:
        t.update(means3D=raw["xyz"], opacities=raw["opacity"], scales=raw["scaling"], rotations=raw["rotation"], d_xyz=raw["d_xyz"],
                 d_rotation=raw["d_rotation"], d_scaling=raw["d_scaling"], shs=raw["features_dc"], shs_rest=raw["features_rest"])
    else:
        t.update(means3D=s["means3D"], opacities=s["opac"], scales=s["scales"], rotations=s["rots"], shs=s["shs"])
    return t


def forward_against_oracle(t, c, so):
    ref = R.reference(t, c)
    val, err, amb = R.bounds(t, c)
    assert int(amb.sum()) == 0
    vis = torch.from_numpy(so.radii > 0)
    assert int(vis.sum()) > 10
    T = lambda a: torch.from_numpy(np.asarray(a)).double()  # noqa: E731
    got = {"px": T(so.xy[:, 0]), "py": T(so.xy[:, 1]), "depth": T(so.depths), "conic": T(so.conic_o[:, :3]), "opacity": T(so.conic_o[:, 3]),
           "rgb": T(so.rgb), "cov3D": T(so.cov3D)}
    for k, g in got.items():
        R.assert_within(k, g[vis], ref[k][vis], err[k][vis])
    assert torch.equal(torch.from_numpy(so.clamped.astype(bool))[vis], ref["clamped"][vis])
    lo, hi = R.radius_sets(ref["r3"], err["r3"])
    r = T(so.radii)
    assert bool(((r >= lo) & (r <= hi))[vis].all()) and float((lo != hi)[vis].float().mean()) <= 0.02
    assert bool((r[ref["depth"] <= 0.2 - err["depth"]] == 0).all())


@pytest.mark.parametrize("seed,H,W,N,deg", [(1, 32, 32, 40, 3), (2, 40, 56, 64, 3), (3, 17, 35, 24, 1), (4, 33, 20, 48, 0), (5, 24, 24, 30, 2)])
def test_forward_equals_the_oracles_saved_state(seed, H, W, N, deg):
    s = small_scene(N, H, W, seed, radius=3.0, fovy=0.5)
    cam = s["cam"]
    out, so = RR.forward(s["means3D"].numpy(), s["opac"].numpy(), cam.world_view_transform.numpy(), cam.full_proj_transform.numpy(),
                         cam.camera_center.numpy(), math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), H, W, np.zeros(3, np.float32),
                         shs=s["shs"].numpy(), scales=s["scales"].numpy(), rotations=s["rots"].numpy(), sh_degree=deg)
    forward_against_oracle(scene_tensors(s, False), dict(glue=False, deg=deg, W=W, H=H), so)


@pytest.mark.parametrize("isotropic,mod", [(False, 1.0), (True, 1.0), (False, 0.5)])
def test_forward_with_glue_equals_the_oracles_render_glue_composition(isotropic, mod):
    N, H, W = 64, 40, 56
    sc = synth.make_scene(N, 6, 21, scale=0.06, sh_rest_std=0.3)
    cam = synth.look_at_camera(H, W, radius=3.0, fovy=0.5)
    g = torch.Generator().manual_seed(9)
    raw = dict(sc)
    raw["rotation"] = sc["rotation"] * (0.3 + 2.7 * torch.rand(N, 1, generator=g))
    raw["scaling"] = sc["scaling"][:, :1].contiguous() if isotropic else sc["scaling"]
    raw["d_xyz"] = 0.02 * torch.randn(N, 3, generator=g)
    raw["d_rotation"] = 0.1 * torch.randn(N, 4, generator=g)
    raw["d_scaling"] = 0.2 * torch.exp(sc["scaling"]) * torch.randn(N, 3, generator=g)
    m3, op, scl, rot, shs = O.render_glue(raw["xyz"], raw["features_dc"], raw["features_rest"], raw["scaling"], raw["rotation"], raw["opacity"],
                                          raw["d_xyz"], raw["d_rotation"], raw["d_scaling"], isotropic)
    out, so = RR.forward(m3.numpy(), op.numpy(), cam.world_view_transform.numpy(), cam.full_proj_transform.numpy(), cam.camera_center.numpy(),
                         math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), H, W, np.zeros(3, np.float32), shs=shs.numpy(), scales=scl.numpy(),
                         rotations=rot.numpy(), scale_modifier=mod)
    forward_against_oracle(scene_tensors({"cam": cam}, True, raw), dict(glue=True, iso=isotropic, deg=3, W=W, H=H, mod=mod), so)


# ------------------------------------------------------------------------------------------ reference against the dense splat
@pytest.mark.parametrize("mode", ["sh", "precomp"])
def test_gradients_composed_with_the_dense_splat_equal_its_end_to_end_gradients(mode):
    """The dense splat's own dL/d(NDC, conic, opacity, rgb, depth) are the record; the reference's autograd of the per-Gaussian
    stage must then give the dense splat's end-to-end gradients: two float64 forms, 1e-10 of the array's largest entry."""
    seed, H, W, N = 2, 40, 56, 64
    s = small_scene(N, H, W, seed, radius=3.0, fovy=0.5)
    cam = s["cam"]
    t = scene_tensors(s, False)
    g = torch.Generator().manual_seed(100 + seed)
    gc, gd, ga = (torch.randn(3, H, W, generator=g, dtype=torch.float64), torch.randn(H, W, generator=g, dtype=torch.float64),
                  torch.randn(H, W, generator=g, dtype=torch.float64))
    d = lambda x: x.double().clone().requires_grad_(True)  # noqa: E731
    leaves = {"means3D": d(s["means3D"]), "opacities": d(s["opac"][:, 0]), "means2D": torch.zeros(N, 3, dtype=torch.float64, requires_grad=True)}
    kw = {}
    if mode == "sh":
        leaves.update(scales=d(s["scales"]), rotations=d(s["rots"]), shs=d(s["shs"]))
        kw = dict(shs=leaves["shs"], scales=leaves["scales"], rots=leaves["rotations"])
    else:
        Mm = DS.quat_R(s["rots"].double()) * s["scales"].double()[:, None, :]
        Sg = Mm @ Mm.transpose(1, 2)
        t["cov3D_precomp"] = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).float()
        t["colors_precomp"] = torch.rand(N, 3, generator=g)
        t["scales"] = t["rotations"] = t["shs"] = None
        leaves.update(cov3D_precomp=d(t["cov3D_precomp"]), colors_precomp=d(t["colors_precomp"]))
        kw = dict(colors=leaves["colors_precomp"], cov6=leaves["cov3D_precomp"])
    taps = {}
    out = DS.render(leaves["means3D"], leaves["means2D"], leaves["opacities"], cam.world_view_transform.double(), cam.full_proj_transform.double(),
                    cam.camera_center.double(), t["tanx"], t["tany"], H, W, torch.tensor([0.2, 0.5, 0.9], dtype=torch.float64), deg=3, taps=taps, **kw)
    loss = (out[0] * gc).sum() + (out[1] * gd).sum() + (out[2] * ga).sum()
    names = list(leaves)
    tap_names = ["ndc", "A", "B", "C", "rgb", "depth"]
    gr = torch.autograd.grad(loss, [leaves[k] for k in names] + [taps[k] for k in tap_names], allow_unused=True)
    end = dict(zip(names, gr[:len(names)]))
    tg = {k: (torch.zeros_like(taps[k]) if v is None else v) for k, v in zip(tap_names, gr[len(names):])}
    vis = out[3] > 0
    # the opacity's record entry: it is a leaf of the dense splat, its end-to-end gradient IS dL/d opacity
    rec = torch.cat([tg["ndc"], tg["A"][:, None], tg["B"][:, None], tg["C"][:, None], end["opacities"][:, None], tg["rgb"], tg["depth"][:, None]], 1)
    assert int((vis & (rec != 0).any(1)).sum()) > 20
    ref = R.reference(t, dict(glue=False, deg=3, W=W, H=H), rec, vis)
    if mode == "sh":
        assert torch.equal(ref["clamped"][vis], (taps["rgb"].detach() == 0)[vis])
    pairs = {"dL_dmeans3D": "means3D", "dL_dopacities": "opacities", "dL_dmeans2D": "means2D", "dL_dscales": "scales", "dL_drotations": "rotations",
             "dL_dsh": "shs", "dL_dcov3D": "cov3D_precomp", "dL_dcolors_precomp": "colors_precomp"}
    checked = 0
    for k, r in ref["grads"].items():
        e = end[pairs[k]].reshape(r.shape)
        assert float(e.abs().max()) > 0 or k == "dL_dmeans2D", k
        assert float((r - e).abs().max()) <= 1e-10 * max(float(e.abs().max()), 1e-300), k
        checked += 1
    assert checked == (6 if mode == "sh" else 5)
    # ... and the float64 evaluation of the KERNEL's formulas (the second opinion inside ``bounds``) agrees with autograd
    val = R.bounds(t, dict(glue=False, deg=3, W=W, H=H), rec, vis)[0]
    for k, r in ref["grads"].items():
        assert float((val[k].reshape(r.shape) - r).abs().max()) <= 1e-10 * max(float(r.abs().max()), 1e-300), k


# ------------------------------------------------------------------------ the float32 restatement within every bound, grid-wide
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_float32_restatement_is_within_every_bound(c):
    t, rec, ref, fref, ferr = prepared(c)
    vis = t["vis"]
    for order in (0, 1, 2):
        got = restated(c, t, rec, order)
        assert failing(got, ref) == [], order
        for k in R.FWD_KEYS:
            R.assert_within("%s order %d" % (k, order), got[k].double()[vis], fref[k][vis], ferr[k][vis])
    # the float64 evaluation of the kernel's formulas agrees with the autograd reference (rows of exact zero gradients aside)
    val = R.bounds(t, c, rec, vis, t["clamp_bits"])[0]
    for k, (r, b) in ref.items():
        if not (c["iso"] and k == "dL_drotations"):
            assert float((val[k].reshape(r.shape) - r).abs().max()) <= 1e-10 * max(float(r.abs().max()), 1e-300), k


# ------------------------------------------------------------------------------------------------------------ planted faults
GLUE_ALL = next(c for c in G.GRID if c["glue"] and c["dxyz"] and c["drot"] and c["dscal"] and c["want_dd"] and not c["iso"] and c["cot"] == "random")
ISO_ALL = next(c for c in G.GRID if c["iso"] and c["dscal"])
SH_ALL = next(c for c in G.GRID if c["N"] == 1025 and c["share"] == "all")
FAULT_CASES = [  # fault, the case, the arrays it spoils (all of them must fail, no other may)
    ("clamp_x_ignored", SH_ALL, ["dL_dmeans3D"]),
    ("clamped_colour_not_zeroed", SH_ALL, ["dL_dmeans3D", "dL_dsh", "dL_dsh_rest"]),
    ("sh_dir_dropped", SH_ALL, ["dL_dmeans3D"]),
    ("sh_dir_no_projection", SH_ALL, ["dL_dmeans3D"]),
    ("d_scaling_not_in_s", GLUE_ALL, ["cov3D", "conic", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dd_scaling"]),
    ("dd_scaling_times_exp", GLUE_ALL, ["dL_dd_scaling"]),
    ("raw_scaling_times_s", GLUE_ALL, ["dL_dscales"]),
    ("quat_no_projection", GLUE_ALL, ["dL_drotations"]),
    ("quat_div_one", GLUE_ALL, ["dL_drotations"]),
    ("iso_column0", ISO_ALL, ["dL_dscales"]),
    ("dR_transposed", SH_ALL, ["dL_drotations"]),
    ("conic_B_halved", SH_ALL, ["dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dd_scaling"]),
    ("depth_row", SH_ALL, ["dL_dmeans3D"]),
]


def test_every_fault_has_its_case():
    assert sorted(f for f, _, _ in FAULT_CASES) == sorted(R.FAULTS)


@pytest.mark.parametrize("fault,c,spoiled", FAULT_CASES, ids=[f for f, _, _ in FAULT_CASES])
def test_planted_fault_is_rejected_on_the_array_it_spoils(fault, c, spoiled):
    t, rec, ref, fref, ferr = prepared(c)
    vis = t["vis"]
    good, bad = restated(c, t, rec), restated(c, t, rec, fault=fault)
    failed = failing(bad, ref) + [k for k in R.FWD_KEYS if R.violations(bad[k].double()[vis], fref[k][vis], ferr[k][vis])[0]]
    assert failing(good, ref) == []
    assert sorted(failed) == sorted(k for k in spoiled if k in bad), failed


# --------------------------------------------------------------------------------------------- the gap that was open: the old bars
def old_bars_pass(got, ref, what):
    """tests/test_gpu_raster.py's _grads_close: gpu_util.assert_close(hip, ref, what, REL_TOL, 1e-5)."""
    try:
        GU.assert_close(got.numpy().reshape(ref.shape), ref.numpy(), what, GU.REL_TOL, 1e-5)
    except AssertionError:
        return False
    finally:
        GU.STATS.pop()
    return True


# The planted faults whose spoiled arrays pass the old bars on the grid's "wide" case (N = 3001, about 5 % of the Gaussians hold a
# record, magnitudes over four decades).  Measured: the ignored frustum clamp alone — it spoils the two Gaussians beside the frustum
# that hold a record, at 5e-5 of the array's largest entry.  Every other fault touches every record holder at 5 - 100 % of its own
# gradient and fails the old bars too (the SH direction term: 3.6 % of the elements beyond 1e-4 of the maximum).
PASS_OLD_BARS = ("clamp_x_ignored",)


def test_faults_that_pass_the_old_bars_fail_the_bounds():
    c = next(c for c in G.GRID if c["cot"] == "wide" and c["N"] == 3001)
    t, rec, ref, fref, ferr = prepared(c)
    good = restated(c, t, rec)
    for k, (r, b) in ref.items():
        assert old_bars_pass(good[k], r, k), k
    passed = []
    for fault in R.FAULTS:
        if fault in ("d_scaling_not_in_s", "dd_scaling_times_exp", "raw_scaling_times_s", "quat_no_projection", "quat_div_one", "iso_column0"):
            continue  # (glue faults: the case has activated inputs)
        bad = restated(c, t, rec, fault=fault)
        spoiled = failing(bad, ref)
        assert spoiled, fault
        if all(old_bars_pass(bad[k], ref[k][0], k) for k in ref):
            passed.append(fault)
    print("planted faults that pass the old bars:", passed)
    assert sorted(passed) == sorted(PASS_OLD_BARS)


# ------------------------------------------------------------------------------------------------------------- non-vacuity
SHARES = {}


def vacuity(c):
    """Per array: (elements counted, share of them whose bound is at least |reference|).  Not counted: elements whose bound is 0
    (compared exactly), and the two quantities of an isotropic Gaussian that are exactly zero in exact arithmetic — its rotation
    gradient and the off-diagonal entries of its Sigma3D — whose reference is ~ 1e-17 and whose bound is their rounding magnitude."""
    t, rec, ref, fref, ferr = prepared(c)
    vis = t["vis"]
    out = {}
    for k, (r, b) in ref.items():
        if c["iso"] and k == "dL_drotations":
            continue
        out[k] = (int((b > 0).sum()), R.vacuity(r, b))
    for k in R.FWD_KEYS:
        r, b = fref[k][vis], ferr[k][vis]
        if c["iso"] and k == "cov3D":
            r, b = r[:, [0, 3, 5]], b[:, [0, 3, 5]]
        out[k] = (int((b > 0).sum()), R.vacuity(r, b))
    return out


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_bounds_are_not_vacuous_on_the_gpu_grid(c):
    sh = vacuity(c)
    SHARES[G.case_id(c)] = sh
    print({k: "%d: %.4f" % v for k, v in sh.items()})
    for k, (n, share) in sh.items():
        assert share <= GAUSS_CAP, (k, n, share)
