"""CPU: the float64 reference of the rasterizer's compositing stage (tests/raster_comp_ref.py) and its bounds, checked on the host.

  * every case of the GPU grid builds: designed list lengths, no ambiguous (pixel, instance) pair, what its scene kind promises;
  * the backward's closed form (prefix / suffix with the background term) and the float64 evaluation of the kernel's own steps
    agree with autograd to 1e-10;
  * the float32 restatement of the kernels' steps stays inside every bound on every grid case, in three groupings / orders, and
    makes the reference's decisions (n_contrib exact);
  * planted faults, each its own case, rejected on the arrays it spoils; and the one the old bars (gpu_util.assert_close as
    tests/test_gpu_raster.py calls it) let through;
  * the bounds are not vacuous on the grid;
  * tests/dense_splat.py fed the same records through its taps gives the reference's image and gradients to 1e-10."""
import math

import pytest
import torch

from tests import dense_splat as DS
from tests import gpu_util as GU
from tests import raster_comp_ref as R
from tests import test_gpu_raster_comp_f64 as G
from tests.test_oracle_raster import small_scene

CAP = 0.10  # the cap of tests/test_raster_gauss_ref_cpu.py: the share of counted elements whose bound is at least |reference|
ALL = G.GRID + [G.TIGHT]
IDS = [c["name"] for c in ALL]
ARRAYS = R.IMG_KEYS + ("rows_geom", "rows_rgb", "rows_depth")

_cache = {}


def prepared(c, kind="random", given=True):
    """(tensors, call arguments, cotangent, reference, bounds, values) of a grid case and a cotangent."""
    key = (c["name"], c["seed"], kind, given)
    if key not in _cache:
        if len(_cache) > 24:
            _cache.pop(next(iter(_cache)))
        t = G.build(c)
        cot = G.make_cot(kind, c, torch.Generator().manual_seed(c["seed"] + 7 + 13 * G.COT_KINDS.index(kind) + given), given)
        a = (t["records"], t["ranges"], t["point_list"], t["bg"], c["H"], c["W"])
        ref = R.reference(*a, cot)
        err, val, amb = R.bounds(*a, ref, cot)
        assert amb == 0
        _cache[key] = (t, a, cot, ref, err, val)
    return _cache[key]


def arrays(o):
    d = {k: o[k].double() for k in R.IMG_KEYS}
    d["rows_geom"], d["rows_rgb"], d["rows_depth"] = o["rows"][:, :6].double(), o["rows"][:, 6:9].double(), o["rows"][:, 9].double()
    return d


def failing(got, ref, err):
    g, r, e = arrays(got), arrays(ref), arrays(err)
    bad = [k for k in ARRAYS if R.violations(g[k], r[k], e[k])[0]]
    if not torch.equal(got["n_contrib"], ref["n_contrib"]):
        bad.append("n_contrib")
    return sorted(bad)


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------ the grid, the restatement in its bounds
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_float32_restatement_is_within_every_bound(c):
    for i, (kind, given) in enumerate(G.cot_plan(c)):
        t, a, cot, ref, err, val = prepared(c, kind, given)
        if kind != "zero":
            assert float(ref["rows"].abs().max()) > 0
        # the closed form of the backward, and the float64 evaluation of the kernel's own steps, against autograd
        assert rel(ref["rows_closed"], ref["rows"]) <= 1e-10, (kind, given)
        assert rel(val["rows"], ref["rows"]) <= 1e-10, (kind, given)
        outs = []
        for order in ((0, 1, 2) if i < 2 else (i % 3,)):  # every order on the case's first two cotangents, one on the others
            got = R.kernel_steps(R.F32(order), *a, cot)
            assert failing(got, ref, err) == [], (kind, given, order)
            outs.append(got)
            for tl, r0, r1 in R.tiles_of(t["ranges"], c["H"], c["W"]):  # untouched instances and rows behind the walk limit: exactly 0
                dead = ~ref["walk"][tl]["use"].any(0)
                dead[ref["tile_max"][tl]:] = True
                assert bool((got["rows"][r0:r1][dead] == 0).all())
        if kind == "random" and c["layout"] == "B":  # the three restatements are three different evaluations
            assert not torch.equal(outs[0]["color"], outs[1]["color"]) and not torch.equal(outs[0]["rows"], outs[1]["rows"])
            assert not torch.equal(outs[0]["rows"], outs[2]["rows"])


def test_checkpoints_of_the_restatement_are_the_references():
    """The exclusive state at every 64th instance: the restatement's checkpoints (both groupings) against the reference's, per
    element within the analysis' own bound of that prefix (the transmittance product and the any-order prefix sums the backward is
    seeded with), where the pixel's walk reaches the chunk; a checkpoint taken one instance late falls outside."""
    c = G.BY_NAME["opaque-B-full"]
    t, a, cot, ref, err, val = prepared(c)

    def outside(got):
        n = bad = 0
        for tl, (ck, valid) in got["ckpt"].items():
            if tl not in ref["ckpt"]:
                continue
            assert torch.equal(valid, ref["ckpt_valid"][tl])
            m = valid[:, None, :].expand_as(ck)
            bad += int(((ck.double() - ref["ckpt"][tl]).abs() > err["ckpt"][tl])[m].sum())
            n += int(m.sum())
        assert n > 10000
        return bad

    for order in (0, 1):
        assert outside(R.kernel_steps(R.F32(order), *a, cot)) == 0, order
    assert outside(R.kernel_steps(R.F32(0), *a, cot, fault="ckpt_late")) > 100


def test_default_mode_columns_through_the_per_gaussian_stage():
    """The four accumulator columns that reach no output unchanged (conic A, B, C, depth): the restatement's float32 sums per
    Gaussian, run through the float32 restatement of the per-Gaussian backward, stay inside that stage's bounds when the reference's
    sums are its record and their bounds the record's error."""
    c = G.BY_NAME["clamped-B-cut"]
    t, a, cot, ref, err, val = prepared(c)
    N = t["N"]
    vis = torch.ones(N, dtype=torch.bool)
    s, e = R.gaussian_sums(ref["rows"], err["rows"], t["point_list"], N)
    gref, gerr = G.per_gaussian_reference(c, t, s, e, vis, True)
    cfg = dict(glue=False, deg=0, W=c["W"], H=c["H"])
    for order in (0, 2):
        rows = R.kernel_steps(R.F32(order), *a, cot)["rows"]
        rec32 = torch.zeros(N, 10).index_add_(0, t["point_list"].long(), rows)
        with torch.no_grad():
            o = G.RG.kernel_steps(G.RG.F32(order), t, cfg, rec=rec32)
        got = G.RG.collect(o, True, vis & (rec32 != 0).any(1))
        for k in ("dL_dcov3D", "dL_dmeans3D"):
            R.assert_within(k, got[k].double().reshape(gref[k].shape), gref[k], gerr[k])
            assert R.vacuity(gref[k], gerr[k]) <= CAP, k
    # the record's error is what decides: with the sums taken as exact the same numbers fall outside
    _, exact, _ = G.RG.bounds(t, cfg, s, vis)
    assert R.violations(got["dL_dcov3D"].double(), gref["dL_dcov3D"], exact["dL_dcov3D"].reshape(N, 6))[0] > 0


# ------------------------------------------------------------------------------------------------------------ planted faults
ALL3 = ["rows_depth", "rows_geom", "rows_rgb"]
EVERY = sorted(ARRAYS + ("n_contrib",))
FAULT_CASES = [  # fault, the case, the restatement's order, the arrays it spoils (all of them must fail, no other may)
    ("stop_on_T", "opaque-B-full", 0, EVERY),
    ("thr_256", "opaque-B-full", 0, EVERY),
    ("clamp_blocks_grad", "clamped-B-cut", 0, ["rows_geom"]),
    ("final_T_behind", "opaque-B-full", 0, ["color", "final_T", "rows_geom"]),
    ("n_contrib_counts_stop", "opaque-B-full", 0, ALL3 + ["n_contrib"]),
    ("ckpt_late", "translucent-A-full", 0, ALL3),
    ("bg_dropped", "mixed-B-cut", 0, ["rows_geom"]),
    ("gA_1mT_dropped", "translucent-A-full", 0, ["rows_geom"]),
    ("pair_dx", "clamped-B-cut", 0, ALL3),
    ("depth_by_colour", "translucent-A-full", 0, ["rows_depth"]),
    ("part_left_out", "mixed-B-cut", 0, ALL3),
    ("wide_other_half", "opaque-B-full", 1, EVERY),
    ("ckpt_late_last", "mixed-B-cut", 0, ALL3),
]


def test_every_fault_has_its_case():
    assert sorted(f for f, _, _, _ in FAULT_CASES) == sorted(R.FAULTS)


@pytest.mark.parametrize("fault,name,order,spoiled", FAULT_CASES, ids=[f[0] for f in FAULT_CASES])
def test_planted_fault_is_rejected_on_the_arrays_it_spoils(fault, name, order, spoiled):
    t, a, cot, ref, err, val = prepared(G.BY_NAME[name])
    assert failing(R.kernel_steps(R.F32(order), *a, cot), ref, err) == []
    assert failing(R.kernel_steps(R.F32(order), *a, cot, fault=fault), ref, err) == sorted(spoiled)


# --------------------------------------------------------------------------------------------- the gap that was open: the old bars
def old_bars_pass(got, ref, what):
    """tests/test_gpu_raster.py's _grads_close: gpu_util.assert_close(hip, ref, what, REL_TOL, 1e-5)."""
    try:
        GU.assert_close(got.numpy(), ref.numpy(), what, GU.REL_TOL, 1e-5)
    except AssertionError:
        return False
    finally:
        GU.STATS.pop()
    return True


# The planted faults that pass the old bars on every array of the grid's opaque-B-full case under the "wide" cotangent (magnitudes
# over four decades from pixel to pixel, everything given) and fail the bounds.  Measured: the checkpoint taken one instance late
# for ONE chunk of the scene (the last used chunk of the 700-instance list).  It spoils 25 elements of the geometry columns, 18 of
# the colour columns and 6 of the depth column, each by less than 1e-4 of its array's largest entry: the rows of instances deep in
# a saturating list are small.  (The clamped and the mixed long case let it through as well; under the "random" cotangent one
# of the three row arrays catches it.)  Every other fault moves some element of its array by more than 1e-4 of the maximum on
# scenes this small and fails the old bars too.
PASS_OLD_BARS = ("ckpt_late_last",)


def test_faults_that_pass_the_old_bars_fail_the_bounds():
    t, a, cot, ref, err, val = prepared(G.BY_NAME["opaque-B-full"], "wide", True)
    r = arrays(ref)
    good = arrays(R.kernel_steps(R.F32(0), *a, cot))
    for k in ARRAYS:
        assert old_bars_pass(good[k], r[k], k), k
    passed = []
    for fault in R.FAULTS:
        bad = R.kernel_steps(R.F32(1 if fault == "wide_other_half" else 0), *a, cot, fault=fault)
        if not failing(bad, ref, err):
            continue  # (a fault that this scene does not exercise)
        b = arrays(bad)
        if all(old_bars_pass(b[k], r[k], k) for k in ARRAYS) and float((bad["n_contrib"] != ref["n_contrib"]).double().mean()) <= 5e-6:
            passed.append(fault)
    print("planted faults that pass the old bars:", passed)
    assert sorted(passed) == sorted(PASS_OLD_BARS)


# ------------------------------------------------------------------------------------------------------------- non-vacuity
SHARES = {}


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_bounds_are_not_vacuous_on_the_gpu_grid(c):
    """Per array and case: of the elements with a bound > 0 (the others are compared exactly), at most CAP have a bound that is
    at least |reference|."""
    for kind, given in G.cot_plan(c):
        if kind == "zero":
            continue
        t, a, cot, ref, err, val = prepared(c, kind, given)
        r, e = arrays(ref), arrays(err)
        sh = {k: (int((e[k] > 0).sum()), R.vacuity(r[k], e[k])) for k in ARRAYS}
        SHARES[(c["name"], kind, given)] = sh
        print(kind, given, {k: "%d: %.4f" % v for k, v in sh.items()})
        for k, (n, share) in sh.items():
            if k == "rows_depth" and not given:
                continue  # (dL_ddepth NULL: the column is exactly zero, nothing is counted)
            assert share <= CAP, (kind, given, k, n, share)


# ------------------------------------------------------------------------------------------ the two float64 references tied together
def test_dense_splat_fed_the_same_records_agrees_with_the_reference():
    """tests/dense_splat.render (no tiles, its own loop over Gaussians) on a small scene; the per-Gaussian tensors it composites come
    out through ``taps`` and are the reference's records; its image and its gradients with respect to the taps must be the
    reference's image and the per-Gaussian sums of the reference's rows: 1e-10 of the array's largest entry."""
    seed, H, W, N = 2, 40, 56, 64
    s = small_scene(N, H, W, seed, radius=3.0, fovy=0.5)
    cam = s["cam"]
    d = lambda x: x.double().clone().requires_grad_(True)  # noqa: E731
    g = torch.Generator().manual_seed(300 + seed)
    bg = torch.tensor([0.2, 0.5, 0.9], dtype=torch.float64)
    opac = (0.85 * s["opac"][:, 0].double()).requires_grad_(True)  # (below the clamp: dense_splat clamps at the double 0.99)
    taps = {}
    out = DS.render(d(s["means3D"]), torch.zeros(N, 3, dtype=torch.float64), opac, cam.world_view_transform.double(), cam.full_proj_transform.double(),
                    cam.camera_center.double(), math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), H, W, bg, shs=d(s["shs"]), scales=d(s["scales"]),
                    rots=d(s["rots"]), deg=3, taps=taps)
    col, dep, alp, radii, ncontrib, Tfin = out
    cot = {"color": torch.randn(3, H, W, generator=g, dtype=torch.float64), "depth": torch.randn(H, W, generator=g, dtype=torch.float64),
           "alpha": torch.randn(H, W, generator=g, dtype=torch.float64)}
    loss = (col * cot["color"]).sum() + (dep * cot["depth"]).sum() + (alp * cot["alpha"]).sum()
    names = ["ndc", "A", "B", "C", "opacity", "rgb", "depth"]
    tg = dict(zip(names, torch.autograd.grad(loss, [opac if k == "opacity" else taps[k] for k in names], allow_unused=True)))
    ndc = taps["ndc"].detach()
    px, py = ((ndc[:, 0] + 1) * W - 1) * 0.5, ((ndc[:, 1] + 1) * H - 1) * 0.5
    records = torch.cat([px[:, None], py[:, None], taps["depth"].detach()[:, None], taps["A"].detach()[:, None], taps["B"].detach()[:, None],
                         taps["C"].detach()[:, None], opac.detach()[:, None], taps["rgb"].detach()], 1)
    # the tile lists of dense_splat's rectangles, ordered by the fp32 depth bits as it orders them
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rad = radii.double()
    vis = radii > 0
    x0, x1 = torch.clamp(torch.trunc((px - rad) / 16), 0, gx), torch.clamp(torch.trunc((px + rad + 15) / 16), 0, gx)
    y0, y1 = torch.clamp(torch.trunc((py - rad) / 16), 0, gy), torch.clamp(torch.trunc((py + rad + 15) / 16), 0, gy)
    order = torch.argsort(taps["depth"].detach().float(), stable=True)
    lists, ranges = [], []
    for tl in range(gx * gy):
        tx, ty = tl % gx, tl // gx
        ids = [int(k) for k in order if bool(vis[k]) and x0[k] <= tx < x1[k] and y0[k] <= ty < y1[k]]
        ranges.append((len(lists), len(lists) + len(ids)) if ids else (0, 0))
        lists += ids
    ranges, pl = torch.tensor(ranges, dtype=torch.int32), torch.tensor(lists, dtype=torch.int32)
    assert pl.numel() > N
    ref = R.reference(records, ranges, pl, bg, H, W, cot)
    for tl, r0, r1 in R.tiles_of(ranges, H, W):  # (no pair at the clamp: the two references clamp at different roundings of 0.99)
        pxl, pyl, inside = R.tile_pixels(tl, H, W)
        assert not bool((R._walk64(records[pl.long()[r0:r1]], pxl.double(), pyl.double(), inside)["alpha"] >= 0.989).any())
    for k, v in (("color", col), ("depth", dep), ("alpha", alp), ("final_T", Tfin)):
        assert rel(ref[k], v.detach()) <= 1e-10, k
    assert torch.equal(ref["n_contrib"], ncontrib)
    sums = torch.zeros(N, 10, dtype=torch.float64).index_add_(0, pl.long(), ref["rows"])
    want = torch.cat([tg["ndc"], tg["A"][:, None], tg["B"][:, None], tg["C"][:, None], tg["opacity"][:, None], tg["rgb"], tg["depth"][:, None]], 1)
    for j in range(10):
        assert float(want[:, j].abs().max()) > 0
        assert rel(sums[:, j], want[:, j]) <= 1e-10, j
    assert rel(ref["rows_closed"], ref["rows"]) <= 1e-10
