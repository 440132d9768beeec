"""-m gpu: the rasterizer's per-Gaussian stage (csrc/preprocess.hip) pinned per element to float64 (tests/raster_gauss_ref.py),
through the C ABI.

Forward: riggs_raster_preprocess + riggs_raster_render as ``rasterize_forward`` issues them, then the per-Gaussian state of the
geometry arena (``saved_views``) against the reference within its bounds, for every visible Gaussian.

Backward BY INJECTION: the test owns a zero-filled workspace of riggs_raster_backward_workspace_bytes(N), writes the cotangent
records of the Gaussians it chooses into the accumulators at its front (csrc/raster_internal.h: PreBwdArgs::gacc) and calls
riggs_raster_backward with a zero dL_dcolor and NULL dL_ddepth / dL_dalpha: the compositing backward adds exact zeros and
preprocess_bwd consumes the injected records.  Both launch forms of preprocess_bwd run on every case
(riggs_set_option("preprocess_bwd_lean", 0 / 1)).  Every output is a view in front of a NaN tail and is pre-filled with NaN (the
header promises "fully written"); per-Gaussian inputs carry a NaN tail; the accumulators must be all zero again on return.  No
record is injected into an invisible Gaussian: the kernel neither reads nor clears it.

The ordered mode (cfg.deterministic) overwrites the accumulators with its own sum, so nothing can be injected; it changes only the
compositing sum and runs the same per-Gaussian code: left out.

GRID is a plain list of dicts and ``build`` makes every tensor from a seeded CPU generator — and asserts on the host that no
Gaussian of the case is ambiguous and that every forced class has its members —: tests/test_raster_gauss_ref_cpu.py imports both
and shows on the host that the bounds hold for a float32 restatement, reject planted faults and are not vacuous on these cases."""
import ctypes as C
import math

import pytest
import torch

from riggs_amd import _lib as L
from riggs_amd import synth
from tests import gpu_util as GU
from tests import raster_gauss_ref as R
from tests.gpu_util import TAIL, in_buf, out_buf

pytestmark = pytest.mark.gpu

H, W = 40, 56  # ragged: 3 x 4 tiles, the last row and column cut
COT_KINDS = ["random", "same_sign", "sparse", "zero", "last", "wide"]
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025, 3001]
CLASSES = ("clamp_x", "clamp_y", "clamp_xy", "near", "col1", "col2", "col3", "aniso")
STRADDLE_CAP = 1e-3


# seeds replaced on the host (check_case: a radius bound that straddles an integer, or an ambiguous decision): case number -> salt
RESEED = {1: 1, 18: 1, 21: 1, 22: 1, 41: 1, 44: 1}  # (all six: one radius bound astride an integer)


def case(N, i, **kw):
    c = dict(N=N, glue=bool(i & 1), iso=False, deg=3, M=16, split=bool(i & 2), cov_pre=False, col_pre=False, dxyz=False, drot=False,
             dscal=False, want_dd=False, mod=1.0, share="all", cot="random", layout="classes", seed=7000 + i + 1000 * RESEED.get(i, 0), H=H, W=W)
    c.update(kw)
    assert c["glue"] or not (c["iso"] or c["dxyz"] or c["drot"] or c["dscal"] or c["want_dd"])
    return c


def _grid():
    cases = []

    def add(N, **kw):
        cases.append(case(N, len(cases), **kw))

    for N in COUNTS:  # counts: one thread, one wave -+ 1, one block -+ 1, several blocks, a ragged last block
        add(N, share="all" if N < 1025 else "some")
    for share in ("none", "one", "some", "all"):  # the share of Gaussians with a record
        add(1025, glue=True, share=share)
    # the staging threshold of the 256-thread form (n_work > 64): 64 records on one wave of a block, 65 spread over its four
    add(512, glue=True, layout="plain", share="wave64", split=False)
    add(512, glue=True, layout="plain", share="spread65", split=True)
    add(512, glue=False, layout="plain", share="spread64", split=False)
    add(512, glue=False, layout="plain", share="wave64+1", split=True)
    # modes
    add(257, glue=False)
    add(257, glue=True)
    add(257, glue=True, iso=True)
    add(257, glue=True, iso=True, dxyz=True, drot=True, dscal=True, want_dd=True)
    add(257, glue=True, dxyz=True)
    add(257, glue=True, drot=True)
    add(257, glue=True, dscal=True)
    add(257, glue=True, dscal=True, want_dd=True)
    add(257, glue=True, want_dd=True)
    add(1025, glue=True, dxyz=True, drot=True, dscal=True, want_dd=True, share="some")
    add(257, glue=False, cov_pre=True)
    add(257, glue=False, col_pre=True)
    add(257, glue=False, cov_pre=True, col_pre=True)
    add(257, glue=True, col_pre=True, dxyz=True)
    for deg in range(4):  # SH degrees in both layouts, with all 16 coefficients stored and with only the active ones
        for split in (False, True):
            add(257, deg=deg, M=16, split=split, glue=bool(deg & 1))
    for deg, split in ((0, False), (1, False), (1, True), (2, False), (2, True)):
        add(257, deg=deg, M=(deg + 1) ** 2, split=split, glue=not (deg & 1))
    add(257, glue=True, mod=0.5)
    add(257, glue=False, mod=0.5)
    for kind in COT_KINDS[1:]:
        add(1025, glue=True, cot=kind, dxyz=True, dscal=True, want_dd=True)
    add(3001, glue=False, cot="wide", share="some")
    return cases


GRID = _grid()
SPARSE_ZERO = [case(1025, 90, glue=True, dxyz=True, drot=True, share="some"), case(257, 91, glue=True, iso=True, split=True, share="some")]
GUARD = case(257, 95, glue=False, col_pre=True, share="some")


def case_id(c):
    return "N%d-%s%s-d%dM%d%s%s%s%s%s%s%s-%s-%s-%s" % (
        c["N"], "glue" if c["glue"] else "act", "-iso" if c["iso"] else "", c["deg"], c["M"], "s" if c["split"] else "", "-cov" if c["cov_pre"] else "",
        "-col" if c["col_pre"] else "", "-dx" if c["dxyz"] else "", "-dr" if c["drot"] else "", "-ds" if c["dscal"] else "",
        "-dd" if c["want_dd"] else "", "mod%g" % c["mod"], c["share"], c["cot"])


_CAM = []


def camera():
    if not _CAM:
        _CAM.append(synth.look_at_camera(H, W))
    return _CAM[0]


def _record_rows(c, vis, g, cls):
    """Which Gaussians receive a record (a subset of the visible ones; "some": about 5 %, one of every forced class among them)."""
    N = c["N"]
    has = torch.zeros(N, dtype=torch.bool)
    share = c["share"]
    if share == "all":
        has[:] = True
    elif share == "some":
        has = torch.rand(N, generator=g) < 0.05
        has[int(torch.nonzero(vis)[-1])] = True
        for rows in cls.values():
            has[rows[:1]] = True
    elif share == "one":
        has[int(torch.nonzero(vis)[len(torch.nonzero(vis)) // 2])] = True
    elif share == "wave64":
        has[256 + 64:256 + 128] = True
    elif share == "wave64+1":
        has[256 + 128:256 + 192] = True
        has[256 + 7] = True
    elif share in ("spread65", "spread64"):
        n = 65 if share == "spread65" else 64
        rows = 256 + torch.cat([w * 64 + torch.randperm(64, generator=g)[:k] for w, k in enumerate((16, 16, 16, n - 48))])
        has[rows] = True
    else:
        assert share == "none"
    return has & vis


def mask_rows(rec, rows):
    """``rec`` with every row outside ``rows`` +0.0 (a product with a 0 / 1 mask would leave -0.0 behind)."""
    return torch.where(rows[:, None], rec, torch.zeros_like(rec)).contiguous()


def _cot(N, kind, g):
    rec = torch.randn(N, 10, generator=g)
    if kind == "same_sign":
        rec = 1 + 0.3 * rec
    elif kind == "sparse":
        rec = torch.where(torch.rand(N, 10, generator=g) < 0.2, rec, torch.zeros_like(rec))
    elif kind == "zero":
        rec = torch.zeros_like(rec)
    elif kind == "last":
        rec[:-1] = 0
    elif kind == "wide":  # magnitudes over four decades from Gaussian to Gaussian, as the compositing's alpha T weights leave them
        rec = rec * torch.pow(10.0, -4.0 * torch.rand(N, 1, generator=g))
    return rec.contiguous()


def build(c, check=True):
    """Every tensor of case ``c`` on the CPU (float32), the decisions of the float32 restatement (``vis``, ``clamp_bits``: what a
    host test uses where a GPU test has the kernel's), the record rows ``has`` and the records ``rec`` (zero outside ``has``)."""
    g = torch.Generator().manual_seed(c["seed"])
    N, glue = c["N"], c["glue"]
    cam = camera()
    view, proj = cam.world_view_transform, cam.full_proj_transform
    tanx, tany = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    k = 0 if c["layout"] == "plain" else (16 if N >= 255 else N // 16)
    perm = torch.randperm(N, generator=g)
    cls = {name: perm[j * k:(j + 1) * k] for j, name in enumerate(CLASSES)}
    # positions in view space
    tz = 2.0 + 4.0 * rnd(N)
    ax, ay = (2 * rnd(N) - 1) * 0.9 * tanx, (2 * rnd(N) - 1) * 0.9 * tany
    sgn = lambda n: torch.sign(rnd(n) - 0.5)  # noqa: E731
    beyond = lambda n, tan: sgn(n) * (1.4 + 0.3 * rnd(n)) * tan  # noqa: E731  (past the 1.3 tan(fov) clamp, 11 - 20 px off the image)
    for name in ("clamp_x", "clamp_xy"):
        ax[cls[name]] = beyond(k, tanx)
    for name in ("clamp_y", "clamp_xy"):
        ay[cls[name]] = beyond(k, tany)
    big = torch.cat([cls["clamp_x"], cls["clamp_y"], cls["clamp_xy"]])
    tz[big] = 2.5 + rnd(3 * k)
    tz[cls["near"]] = -0.5 + 0.65 * rnd(k)  # behind the near plane (0.2): t_z in [-0.5, 0.15]
    pv = torch.stack([ax * tz, ay * tz, tz], 1)
    V64 = view.double()
    pos = ((pv - V64[3, :3]) @ torch.linalg.inv(V64[:3, :3])).float()
    t = {"view": view.contiguous(), "proj": proj.contiguous(), "campos": cam.camera_center.contiguous(), "tanx": tanx, "tany": tany}
    d_xyz = (0.02 * torch.randn(N, 3, generator=g)) if c["dxyz"] else None
    t["d_xyz"] = d_xyz
    t["means3D"] = (pos - d_xyz if d_xyz is not None else pos).contiguous()
    # scales: from sub-pixel (0.003: 0.05 px) to tile-filling, strongly anisotropic ones, large ones beside the frustum
    sc = torch.exp(math.log(0.003) + (math.log(0.3) - math.log(0.003)) * rnd(N, 1) + 0.3 * torch.randn(N, 3, generator=g, dtype=torch.float64))
    sc[cls["aniso"]] = (0.2 + 0.2 * rnd(k, 1)) * torch.tensor([1.0, 0.01, 0.3], dtype=torch.float64)
    sc[big] = 0.5 + 0.3 * rnd(3 * k, 3)
    if c["iso"]:
        sc = sc[:, :1].expand(N, 3).clone()
    sc = sc / c["mod"]
    q = torch.randn(N, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    if c["cov_pre"]:
        Mm = R.DS.quat_R(q) * sc[:, None, :]
        Sg = Mm @ Mm.transpose(1, 2)
        t["cov3D_precomp"] = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).float().contiguous()
        t["scales"] = t["rotations"] = None
    elif glue:
        d_s = (0.2 * sc * torch.randn(N, 3, generator=g, dtype=torch.float64)) if c["dscal"] else None
        es = sc - d_s if d_s is not None else sc
        t["scales"] = torch.log(es[:, :1] if c["iso"] else es).float().contiguous()
        t["d_scaling"] = None if d_s is None else d_s.float().contiguous()
        d_r = (0.1 * torch.randn(N, 4, generator=g, dtype=torch.float64)) if c["drot"] else None
        v = q * torch.exp(math.log(0.3) + (math.log(3.0) - math.log(0.3)) * rnd(N, 1))  # un-normalised: |v| in [0.3, 3]
        t["rotations"] = (v - d_r if d_r is not None else v).float().contiguous()
        t["d_rotation"] = None if d_r is None else d_r.float().contiguous()
    else:
        t["scales"], t["rotations"] = sc.float().contiguous(), q.float().contiguous()
    opac = 1.5 * torch.randn(N, 1, generator=g)
    t["opacities"] = (opac if glue else torch.sigmoid(opac)).contiguous()
    if c["col_pre"]:
        t["colors_precomp"] = torch.rand(N, 3, generator=g).contiguous()
        t["shs"] = t["shs_rest"] = None
    else:
        shs = 0.15 * torch.randn(N, c["M"], 3, generator=g)
        shs[:, 0] = 0.8 * torch.randn(N, 3, generator=g)
        for n, name in enumerate(("col1", "col2", "col3")):  # one, two, three channels far below zero (0.28 * -6 + 0.5), the others far above
            shs[cls[name], 0] = 2.0 + torch.rand(k, 3, generator=g)
            for j in range(n + 1):
                shs[cls[name], 0, (j + n) % 3] = -6.0 - torch.rand(k, generator=g)
        t["shs"] = (shs[:, :1] if c["split"] and c["M"] > 1 else shs).contiguous()
        t["shs_rest"] = shs[:, 1:].contiguous() if c["split"] and c["M"] > 1 else None
    # decisions of the float32 restatement, the record rows and the records
    with torch.no_grad():
        o32 = R.kernel_steps(R.F32(), t, c)
    vis = o32["vis"]
    t["vis"] = vis
    t["clamp_bits"] = (o32["clamped"].long() * torch.tensor([1, 2, 4])).sum(1).to(torch.uint8)
    t["has"] = _record_rows(c, vis, g, cls) if bool(vis.any()) else torch.zeros(N, dtype=torch.bool)
    t["rec"] = mask_rows(_cot(N, c["cot"], g), t["has"])
    t["cls"] = cls
    t["k"] = k
    if check:
        check_case(c, t)
    return t


def check_case(c, t):
    """On the host, before anything runs on a GPU: no ambiguous Gaussian, the radius bound straddles an integer on at most
    STRADDLE_CAP of the Gaussians, every forced class has its k members (counted by the float64 reference)."""
    ref = R.reference(t, c)
    val, err, amb = R.bounds(t, c)
    assert int(amb.sum()) == 0, "%d ambiguous Gaussians: replace the seed of %s" % (int(amb.sum()), case_id(c))
    lo, hi = R.radius_sets(ref["r3"], err["r3"])
    vis = t["vis"]
    assert float(((lo != hi) & vis).float().mean()) <= STRADDLE_CAP, "radius straddles: replace the seed of " + case_id(c)
    k, cls = t["k"], t["cls"]
    cx, cy = ref["clamp_x"], ref["clamp_y"]
    assert int((vis[cls["clamp_x"]] & cx[cls["clamp_x"]] & ~cy[cls["clamp_x"]]).sum()) == k
    assert int((vis[cls["clamp_y"]] & ~cx[cls["clamp_y"]] & cy[cls["clamp_y"]]).sum()) == k
    assert int((vis[cls["clamp_xy"]] & cx[cls["clamp_xy"]] & cy[cls["clamp_xy"]]).sum()) == k
    assert int((ref["depth"][cls["near"]] <= 0.15).sum()) == k and not bool(vis[cls["near"]].any())
    if not c["col_pre"]:
        ncl = ref["clamped"].sum(1)
        for n, name in enumerate(("col1", "col2", "col3")):
            assert int((ncl[cls[name]] == n + 1).sum()) == k, name
    if not c["cov_pre"] and not c["iso"]:
        s = (torch.exp(t["scales"].double()) + (0 if t.get("d_scaling") is None else t["d_scaling"].double())) if c["glue"] else t["scales"].double()
        assert int((s[cls["aniso"]].abs().max(1).values / s[cls["aniso"]].abs().min(1).values >= 50).sum()) == k
    if c["glue"] and not c["cov_pre"]:
        n = (t["rotations"].double() + (0 if t.get("d_rotation") is None else t["d_rotation"].double())).norm(dim=1)
        assert int(((n - 1).abs() > 0.1).sum()) >= min(16, c["N"] // 2)
    if c["layout"] == "plain":
        assert bool(vis.all())
    if c["share"] in ("wave64", "spread64"):
        assert int(t["has"][256:512].sum()) == 64 and int(t["has"].sum()) == 64
    if c["share"] in ("wave64+1", "spread65"):
        assert int(t["has"][256:512].sum()) == 65 and int(t["has"].sum()) == 65
    if c["share"] in ("some", "all", "one") and c["N"] > 1:
        assert int(t["has"].sum()) >= 1


def reference_of(c, t, rec, vis, clamp_bits):
    """{array: (float64 reference, per-element bound)} of the backward of case ``c`` for the records ``rec``."""
    ref = R.reference(t, c, rec, vis, clamp_bits)
    val, err, amb = R.bounds(t, c, rec, vis, clamp_bits)
    out = {}
    for k, r in ref["grads"].items():
        out[k] = (r, err[k].reshape(r.shape))
    return out


def output_shapes(c):
    N, M = c["N"], c["M"]
    sh = {"dL_dmeans3D": (N, 3), "dL_dmeans2D": (N, 3), "dL_dopacities": (N, 1)}
    if c["col_pre"]:
        sh["dL_dcolors_precomp"] = (N, 3)
    elif c["split"] and M > 1:
        sh["dL_dsh"], sh["dL_dsh_rest"] = (N, 1, 3), (N, M - 1, 3)
    else:
        sh["dL_dsh"] = (N, M, 3)
    if c["cov_pre"]:
        sh["dL_dcov3D"] = (N, 6)
    else:
        sh["dL_dscales"], sh["dL_drotations"] = (N, 1 if c["iso"] else 3), (N, 4)
        if c["want_dd"]:
            sh["dL_dd_scaling"] = (N, 3)
    return sh


INPUTS = ("means3D", "shs", "shs_rest", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp", "d_xyz", "d_rotation", "d_scaling")


class Frame:
    """Device inputs of a case in front of NaN tails, its forward, and the injected backward."""

    def __init__(self, c, t, fill=float("nan")):
        from riggs_amd.rasterizer import rasterize_forward, saved_views
        self.c, self.N = c, c["N"]
        self.inp = {k: (None if t.get(k) is None else in_buf(t[k])) for k in INPUTS}
        i = lambda k: None if self.inp[k] is None else self.inp[k][0]  # noqa: E731
        st = GU.settings_for(camera(), [0.1, 0.3, 0.7], c["deg"], c["mod"], debug=False)
        res = rasterize_forward(st, i("means3D"), i("shs"), i("colors_precomp"), i("opacities"), i("scales"), i("rotations"), i("cov3D_precomp"),
                                d_xyz=i("d_xyz"), d_rotation=i("d_rotation"), d_scaling=i("d_scaling"), glue=c["glue"], isotropic=c["iso"],
                                shs_rest=i("shs_rest"))
        self.radii, self.s = res[1], res[4]
        self.v = saved_views(self.s)
        lib = L.lib()
        self.ws_bytes = int(lib.riggs_raster_backward_workspace_bytes(self.N))
        assert self.ws_bytes >= self.N * 48 and self.ws_bytes % 4 == 0
        self.ws = torch.zeros(self.ws_bytes // 4 + TAIL, dtype=torch.float32, device="cuda")
        self.ws[self.ws_bytes // 4:] = GU.SENT
        self.out = {k: out_buf(sh, fill=fill) for k, sh in output_shapes(c).items()}
        self.zero_color = torch.zeros(3, H, W, dtype=torch.float32, device="cuda")

    def inject(self, rec):
        acc = self.ws[:self.N * 12].view(self.N, 12)
        assert bool((acc == 0).all()), "the accumulators are not zero before the injection"
        acc[:, :10] = rec.cuda()

    def backward(self, sparse_zero=0):
        s, i = self.s, (lambda k: None if self.inp[k] is None else self.inp[k][0].data_ptr())
        o = lambda k: self.out[k][0].data_ptr() if k in self.out else None  # noqa: E731
        cfg = s.cfg
        cfg.sparse_zero, cfg.deterministic = sparse_zero, 0
        L.check(L.lib().riggs_raster_backward(
            C.byref(cfg), i("means3D"), i("shs"), i("shs_rest"), i("colors_precomp"), i("opacities"), i("scales"), i("rotations"),
            i("cov3D_precomp"), i("d_xyz"), i("d_rotation"), i("d_scaling"), s.radii.data_ptr(), s.geom.data_ptr(), s.binning.data_ptr(),
            s.cap, s.img.data_ptr(), s.counters.data_ptr(), self.zero_color.data_ptr(), None, None, self.ws.data_ptr(), o("dL_dmeans3D"),
            o("dL_dmeans2D"), o("dL_dsh"), o("dL_dcolors_precomp"), o("dL_dopacities"), o("dL_dscales"), o("dL_drotations"), o("dL_dcov3D"),
            o("dL_dd_scaling"), o("dL_dsh_rest"), L.stream_ptr()), "riggs_raster_backward")
        torch.cuda.synchronize()

    def after(self, tag, fill_nan=True):
        N = self.N
        assert bool((self.ws[self.ws_bytes // 4:] == GU.SENT).all()), "write past the end of the workspace " + tag
        assert bool((self.ws[:N * 12] == 0).all()), "the accumulators are not all zero again " + tag
        for k, (_, buf) in self.out.items():
            tail = buf[N:]
            assert bool(torch.isnan(tail).all() if fill_nan else (tail == 0).all()), "write past the end of %s %s" % (k, tag)
        for k, pair in self.inp.items():
            if pair is not None:
                assert bool(torch.isnan(pair[1][N:]).all()), "input tail of %s changed %s" % (k, tag)

    def refill(self, value=float("nan")):
        for _, buf in self.out.values():
            buf.fill_(value)


def set_lean(v):
    L.check(L.lib().riggs_set_option(b"preprocess_bwd_lean", int(v)), "riggs_set_option")


def get_lean():
    v = C.c_int32()
    L.check(L.lib().riggs_get_option(b"preprocess_bwd_lean", C.byref(v)), "riggs_get_option")
    return int(v.value)


def check_forward(c, t, f, tag):
    """Every element of every visible Gaussian's state within its bound; radii and clamp bits."""
    ref = R.reference(t, c)
    val, err, amb = R.bounds(t, c)
    v = f.v
    radii = f.radii.cpu()
    vis = radii > 0
    xyd, co, rgb = v["xyd"].cpu(), v["conic_o"].cpu(), v["rgb"].cpu()
    lo, hi = R.radius_sets(ref["r3"], err["r3"])
    assert bool((radii[ref["depth"] <= 0.2 - err["depth"]] == 0).all()), "a Gaussian behind the near plane is visible " + tag
    assert bool((radii[~t["vis"] & (lo == hi)] == 0).all()), "a Gaussian without tiles is visible " + tag
    assert bool(vis[t["vis"] & (lo == hi)].all()), "a Gaussian with tiles is invisible " + tag
    r64 = radii.double()
    assert bool(((r64 >= lo) & (r64 <= hi))[vis].all()), "radius outside the integers its bound admits " + tag
    assert float(((lo != hi) & vis).float().mean()) <= STRADDLE_CAP, tag
    got = {"px": xyd[:, 0], "py": xyd[:, 1], "depth": xyd[:, 2], "conic": co[:, :3], "opacity": co[:, 3], "rgb": rgb[:, :3], "cov3D": v["cov3D"].cpu()}
    worst = {}
    for k, gv in got.items():
        worst[k] = R.assert_within("%s %s" % (k, tag), gv.double()[vis], ref[k][vis], err[k][vis], stats=GU.STATS)
    if not c["col_pre"]:
        bits = (ref["clamped"].long() * torch.tensor([1, 2, 4])).sum(1)
        assert torch.equal(v["clamped"].cpu().long()[vis], bits[vis]), "clamp bits differ " + tag
    return vis, v["clamped"].cpu(), worst


def check_backward(f, ref, tag):
    worst = {}
    for k, (view, _) in f.out.items():
        r, b = ref[k]
        worst[k] = R.assert_within("%s %s" % (k, tag), view.cpu().double().reshape(r.shape), r, b, stats=GU.STATS)
    return worst


WORST = {}  # case id -> {array: worst err / bound} (tools read it after a run; nothing in the tests does)


def run_case(c):
    tag = case_id(c)
    t = build(c)
    f = Frame(c, t)
    vis, clamp_bits, worst = check_forward(c, t, f, tag)
    rec = mask_rows(t["rec"], vis)
    ref = reference_of(c, t, rec, vis, clamp_bits)
    WORST[tag] = {"forward": worst}
    before = get_lean()
    try:
        for lean in (0, 1):
            set_lean(lean)
            f.refill()
            f.inject(rec)
            f.backward()
            f.after("%s lean=%d" % (tag, lean))
            WORST[tag]["lean%d" % lean] = check_backward(f, ref, "%s lean=%d" % (tag, lean))
    finally:
        set_lean(before)


def test_injected_records_pass_through_bit_for_bit():
    """The guard of the injection: with activated inputs and colors_precomp the first two columns of dL_dmeans2D, dL_dopacities and
    dL_dcolors_precomp ARE entries 0, 1, 5 and 6..8 of the record.  A change of the record's layout fails here, loudly."""
    c = GUARD
    t = build(c)
    f = Frame(c, t)
    vis = f.radii.cpu() > 0
    rec = mask_rows(t["rec"], vis)
    assert int((rec != 0).any(1).sum()) >= 4
    before = get_lean()
    try:
        for lean in (0, 1):
            set_lean(lean)
            f.refill()
            f.inject(rec)
            f.backward()
            f.after("guard lean=%d" % lean)
            bits = lambda x: x.contiguous().view(torch.int32)  # noqa: E731
            m2 = f.out["dL_dmeans2D"][0].cpu()
            assert torch.equal(bits(m2[:, :2]), bits(rec[:, :2])), "dL_dmeans2D is not the record's first two entries"
            assert bool((m2[:, 2] == 0).all())
            assert torch.equal(bits(f.out["dL_dopacities"][0].cpu()[:, 0]), bits(rec[:, 5])), "dL_dopacities is not entry 5"
            assert torch.equal(bits(f.out["dL_dcolors_precomp"][0].cpu()), bits(rec[:, 6:9])), "dL_dcolors_precomp is not entries 6..8"
    finally:
        set_lean(before)


@pytest.mark.parametrize("c", GRID, ids=["%d-%s" % (i, case_id(c)) for i, c in enumerate(GRID)])
def test_per_gaussian_stage_against_float64(c):
    run_case(c)


@pytest.mark.parametrize("lean", [0, 1])
@pytest.mark.parametrize("c", SPARSE_ZERO, ids=[case_id(c) for c in SPARSE_ZERO])
def test_sparse_zero_two_calls_on_the_same_buffers(c, lean):
    """cfg.sparse_zero = 1: buffers and workspace zero-filled together, then two calls with different record sets.  Rows with a
    record in the first call and none in the second are rewritten to zero, rows with a record in neither keep their zeros, rows
    with a record in the second are within their bounds."""
    tag = case_id(c) + " sparse_zero lean=%d" % lean
    t = build(c)
    f = Frame(c, t, fill=0.0)
    vis, clamp_bits = f.radii.cpu() > 0, f.v["clamped"].cpu()
    g = torch.Generator().manual_seed(c["seed"] + 1)
    first = mask_rows(t["rec"], vis)
    has2 = (torch.rand(c["N"], generator=g) < 0.08) & vis
    has1 = (first != 0).any(1)
    has2[torch.nonzero(has1)[:3, 0]] = True  # some rows in both calls
    second = mask_rows(torch.randn(c["N"], 10, generator=g), has2)
    assert int((has1 & ~has2).sum()) >= 4 and int((has2 & ~has1).sum()) >= 4 and int((has1 & has2).sum()) >= 3
    before = get_lean()
    try:
        set_lean(lean)
        for rec in (first, second):
            ref = reference_of(c, t, rec, vis, clamp_bits)
            f.inject(rec)
            f.backward(sparse_zero=1)
            f.after(tag, fill_nan=False)
            check_backward(f, ref, tag)  # (rows without a record: reference 0 with bound 0, compared exactly)
    finally:
        set_lean(before)
