"""-m gpu: the rasterizer's compositing stage (csrc/render.hip, csrc/recolor.hip) pinned to float64 per pixel and per tile instance
(tests/raster_comp_ref.py), through the C ABI.

The stage boundary is in memory: after riggs_raster_render the geometry arena holds the float32 records the compositing reads and
the image / binning arenas hold ``ranges`` and ``point_list``.  The reference takes the kernel's OWN records and lists, cast exactly
to float64; what is compared is compositing arithmetic only.  The backward is read at its finest grain: with cfg.deterministic the
compositing backward leaves one row of 10 floats per tile instance behind riggs_raster_backward_workspace_bytes(N) in the workspace
(row = sorted instance index), a sum over at most 256 pixels of one tile, no atomics.  Per Gaussian, the ordered gather's and the
default mode's outputs are held to the float64 sums of the rows: the three outputs that return accumulator columns unchanged
(activated inputs + colors_precomp) directly, dL_dcov3D / dL_dmeans3D through the per-Gaussian stage's reference with the sums'
bounds as the error of its record.

The scenes are AUTHORED: every tile holds small Gaussians whose ceil(3 sigma) rectangle stays inside it (three per scene sit on
the border of two tiles on purpose and are in both lists), so a tile's list has exactly the designed length (asserted against the
kernel's ``ranges``).  ``build`` makes a case on the host from a seeded generator, derives
the records with the float32 restatement of the per-Gaussian stage (tests/raster_gauss_ref.py) and asserts, before anything runs on a
GPU, the designed lengths, that no (pixel, instance) pair is ambiguous and what the scene kind promises (stop residues, clamped
pairs, untouched instances, tile_max < total).  tests/test_raster_comp_ref_cpu.py imports GRID and ``build``."""
import ctypes as C
import math

import pytest
import torch

from riggs_amd import _lib as L
from riggs_amd import synth
from tests import gpu_util as GU
from tests import raster_comp_ref as R
from tests import raster_gauss_ref as RG
from tests.gpu_util import TAIL, in_buf, out_buf

pytestmark = pytest.mark.gpu

LAYOUTS = {"A": (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255), "B": (256, 257, 319, 320, 321, 511, 512, 513, 0, 1, 64, 700)}
SIZES = {"full": (48, 64), "cut": (40, 56)}  # (H, W): 3 x 4 full tiles; the last row and column cut
KINDS = ("translucent", "opaque", "clamped", "sparse", "mixed")
COT_KINDS = ("random", "same_sign", "sparse", "zero", "wide")
DEAD = 0.002  # an opacity below 1/255: the instance is in its tile's list and reaches no pixel
STRADDLE, STRADDLE_TILES = 3, (5, 6)  # Gaussians on the border between tiles 5 and 6 (63 | 64 and 511 | 512 instances), in both lists

# seeds replaced on the host (check_case: an ambiguous pair, or a property of the scene kind that the draw missed): case name -> salt
RESEED = {}


def case(kind, layout, size, bg=(0.1, 0.3, 0.7), tight=False, dead=0.0):
    """``dead``: the share of every list, at random positions, whose opacity is DEAD; ``tight``: cfg.tight_lists = 1."""
    name = "%s-%s-%s%s" % (kind, layout, size, "-tight" if tight else "")
    H, W = SIZES[size]
    return dict(name=name, kind=kind, layout=layout, size=size, H=H, W=W, bg=bg, tight=tight, dead=dead,
                seed=9100 + 17 * KINDS.index(kind) + 5 * "AB".index(layout) + (size == "cut") + 1000 * RESEED.get(name, 0))


GRID = [case(k, lay, "full" if (i + j) % 2 == 0 else "cut") for i, k in enumerate(KINDS) for j, lay in enumerate("AB")]
# cfg.tight_lists drops the instances whose alpha >= 1/255 box reaches no pixel centre of the tile: here the 30 % of every list
# whose opacity is below 1/255, at random list positions — what is left moves up, and with it the grouping and the checkpoints
TIGHT = case("translucent", "B", "cut", tight=True, dead=0.3)
TIGHT_DROP_BELOW, TIGHT_KEEP_ABOVE = 0.003, 0.005  # preprocess_fwd keeps a box for 2 ln(255 o) + 0.05 > 0: o > 0.003825
BY_NAME = {c["name"]: c for c in GRID + [TIGHT]}

_CAM = {}


def camera(c):
    if c["size"] not in _CAM:
        _CAM[c["size"]] = synth.look_at_camera(c["H"], c["W"])
    return _CAM[c["size"]]


def _opacities(kind, L_, g, depth_rank, list_len, dead=0.0):
    u = lambda a, b: a + (b - a) * torch.rand(L_, generator=g, dtype=torch.float64)  # noqa: E731
    if kind == "translucent":
        o = u(0.6, 1.0) * min(0.6, max(0.02, 40.0 / list_len))
        if dead > 0:
            o[torch.rand(L_, generator=g) < dead] = DEAD
        return o
    if kind == "opaque":
        return u(0.3, 0.95)
    if kind == "clamped":
        o = u(0.05, 0.3)
        o[torch.rand(L_, generator=g) < 0.34] = 1.0
        return o
    if kind == "sparse":
        o = u(0.1, 0.6)
        o[torch.rand(L_, generator=g) < 0.85] = DEAD
        return o
    o = u(0.2, 0.9)  # mixed: the deepest 40 % of a list reach no pixel
    o[depth_rank >= int(math.ceil(0.6 * L_))] = DEAD
    return o


def build(c, check=True):
    """The case's CPU tensors: inputs of the C ABI (means3D, cov3D_precomp, colors_precomp, activated opacities), the host state of
    the stage boundary (``records`` (N, 10) float64 of the float32 restatement, ``ranges``, ``point_list``) and ``design``: the
    tile of every Gaussian."""
    g = torch.Generator().manual_seed(c["seed"])
    H, W = c["H"], c["W"]
    cam = camera(c)
    view, proj = cam.world_view_transform, cam.full_proj_transform
    tanx, tany = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    gx = (W + 15) // 16
    lens = LAYOUTS[c["layout"]]
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    # STRADDLE Gaussians sit on the border between two neighbouring tiles and are in both lists: the only rows that meet another
    # tile's in the per-Gaussian sums.  They are the scene's last Gaussians; the two tiles hold that many fewer of their own.
    own = list(lens)
    own[STRADDLE_TILES[0]] -= STRADDLE
    own[STRADDLE_TILES[1]] -= STRADDLE
    tile = torch.cat([torch.full((n,), t, dtype=torch.int64) for t, n in enumerate(own)] + [torch.full((STRADDLE,), STRADDLE_TILES[0], dtype=torch.int64)])
    N = tile.shape[0]
    strad = torch.zeros(N, dtype=torch.bool)
    strad[N - STRADDLE:] = True
    uv = 4.2 + 7.6 * rnd(N, 2)
    if c["kind"] == "clamped":
        uv = torch.round(5.0 + 6.0 * rnd(N, 2)) + 0.02 * (rnd(N, 2) - 0.5)
    uv[strad, 0] = 16.0 + 0.6 * (rnd(STRADDLE) - 0.5)
    cx, cy = (tile % gx) * 16 + uv[:, 0], (tile // gx) * 16 + uv[:, 1]
    z = 2.0 + 4.0 * rnd(N)
    rank = torch.zeros(N, dtype=torch.int64)
    opac = torch.zeros(N, dtype=torch.float64)
    at = 0
    for tl, n in enumerate(own):
        if n:
            rank[at:at + n] = torch.argsort(torch.argsort(z[at:at + n]))
            opac[at:at + n] = _opacities(c["kind"], n, g, rank[at:at + n], lens[tl], c["dead"])
        at += n
    opac[strad] = _opacities(c["kind"], STRADDLE, g, rank[strad], lens[STRADDLE_TILES[0]])
    ndcx, ndcy = (2 * cx + 1) / W - 1, (2 * cy + 1) / H - 1
    pv = torch.stack([ndcx * tanx * z, ndcy * tany * z, z], 1)
    V64 = view.double()
    pos = ((pv - V64[3, :3]) @ torch.linalg.inv(V64[:3, :3])).float()
    fx = W / (2 * tanx)
    s = (0.5 + 0.5 * rnd(N, 1)) * (z[:, None] / fx) * (0.7 + 0.3 * rnd(N, 3))
    q = torch.randn(N, 4, generator=g, dtype=torch.float64)
    Mm = RG.DS.quat_R(q / q.norm(dim=1, keepdim=True)) * s[:, None, :]
    Sg = Mm @ Mm.transpose(1, 2)
    t = {"view": view.contiguous(), "proj": proj.contiguous(), "campos": cam.camera_center.contiguous(), "tanx": tanx, "tany": tany,
         "means3D": pos.contiguous(), "opacities": opac.float()[:, None].contiguous(),
         "cov3D_precomp": torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).float().contiguous(),
         "colors_precomp": torch.rand(N, 3, generator=g).contiguous(), "scales": None, "rotations": None, "shs": None, "shs_rest": None,
         "design": tile, "N": N, "bg": torch.tensor(c["bg"], dtype=torch.float32)}
    # ---- the stage boundary on the host: the float32 restatement of the per-Gaussian stage, the rectangles, the sorted lists
    with torch.no_grad():
        o = RG.kernel_steps(RG.F32(), t, dict(glue=False, deg=0, W=W, H=H))
    assert bool(o["vis"].all())
    f64 = lambda x: x.to(torch.float64)  # noqa: E731
    t["records"] = torch.stack([f64(o["px"]), f64(o["py"]), f64(o["depth"])] + [f64(x) for x in o["conic"]] + [f64(o["opacity"])] +
                               [f64(x) for x in o["rgb"]], 1)
    rad, pxv, pyv = o["radius"].double(), f64(o["px"]), f64(o["py"])
    gy = (H + 15) // 16
    f32t = lambda x: x.float().double()  # noqa: E731
    x0, x1 = torch.trunc(f32t(f32t(pxv - rad) / 16)).clamp(0, gx), torch.trunc(f32t(f32t(f32t(pxv + rad) + 15) / 16)).clamp(0, gx)
    y0, y1 = torch.trunc(f32t(f32t(pyv - rad) / 16)).clamp(0, gy), torch.trunc(f32t(f32t(f32t(pyv + rad) + 15) / 16)).clamp(0, gy)
    assert bool((((x1 - x0 == 1) | strad) & (y1 - y0 == 1)).all()), "a rectangle leaves its tile: " + c["name"]
    assert bool((x1 - x0 == 2)[strad].all()), "a straddler is not in both tiles: " + c["name"]
    assert torch.equal((y0 * gx + x0).long(), tile), "a Gaussian sits in another tile than designed: " + c["name"]
    depth32 = o["depth"].float()
    lists, ranges = [], []
    for tl in range(gx * gy):
        tx, ty = tl % gx, tl // gx
        ids = torch.nonzero((x0 <= tx) & (tx < x1) & (y0 <= ty) & (ty < y1))[:, 0]
        ids = ids[torch.argsort(depth32[ids], stable=True)]  # (depth bits, ties by ascending index)
        if c["tight"]:  # (every kept Gaussian's box reaches the tiles of its rectangle: asserted against the kernel's ranges)
            ids = ids[opac[ids] > TIGHT_KEEP_ABOVE]
        n0 = sum(x.numel() for x in lists)
        ranges.append((n0, n0 + ids.numel()) if ids.numel() else (0, 0))
        lists.append(ids)
    t["point_list"] = torch.cat(lists).to(torch.int32)
    t["ranges"] = torch.tensor(ranges, dtype=torch.int32)
    t["straddlers"] = strad
    assert not bool(((opac > TIGHT_DROP_BELOW) & (opac < TIGHT_KEEP_ABOVE)).any())
    t["lens"] = tuple(x.numel() for x in lists)  # the designed lengths; with tight lists, what is left of them
    if c["tight"]:
        assert sum(t["lens"]) < sum(lens) and any(n >= 64 and m < n for n, m in zip(lens, t["lens"])), "tight lists drop nothing"
        assert any(m >= 64 for m in t["lens"])
        # ... and some in front of the first chunk boundary of a long list, so that every later checkpoint sits at another instance
        gone = [opac[ids] <= TIGHT_KEEP_ABOVE for ids in tight_full_lists(x0, x1, y0, y1, gx, gy, depth32)]
        assert any(n >= 128 and bool(d[:64].any()) for d, n in zip(gone, lens)), "no instance is dropped in front of a checkpoint"
    if check:
        check_case(c, t)
    return t


def tight_full_lists(x0, x1, y0, y1, gx, gy, depth32):
    """The canonical (not tight) list of every tile: what the tight case's lists are cut from."""
    out = []
    for tl in range(gx * gy):
        tx, ty = tl % gx, tl // gx
        ids = torch.nonzero((x0 <= tx) & (tx < x1) & (y0 <= ty) & (ty < y1))[:, 0]
        out.append(ids[torch.argsort(depth32[ids], stable=True)])
    return out


_REF = {}


def host_reference(c, t):
    key = c["name"] + str(c["seed"])
    if key not in _REF:
        if len(_REF) > 3:
            _REF.pop(next(iter(_REF)))
        ref = R.reference(t["records"], t["ranges"], t["point_list"], t["bg"], c["H"], c["W"])
        err, _, amb = R.bounds(t["records"], t["ranges"], t["point_list"], t["bg"], c["H"], c["W"], ref)
        _REF[key] = (ref, err, amb)
    return _REF[key]


def check_scene(c, ref, lens, tiles):
    """What the scene kind promises, counted on a reference's decisions (the host's, and again the kernel's own records')."""
    kind = c["kind"]
    walks = ref["walk"]
    stops = torch.cat([w["stop_pos"][w["stopped"]] for w in walks.values()]) if walks else torch.zeros(0, dtype=torch.int64)
    if kind == "translucent":
        assert stops.numel() == 0, "a pixel stops in the translucent scene " + c["name"]
        for t, r0, r1 in tiles:
            if r1 - r0 >= 8:
                assert ref["tile_max"][t] >= (r1 - r0) - 8, (c["name"], t)  # the walk is as deep as the list
    if kind == "opaque":
        assert stops.numel() >= 8, "hardly a pixel saturates in the opaque scene " + c["name"]
    if kind == "opaque" and c["layout"] == "B":
        assert set((stops % 8).tolist()) == set(range(8)) and set((stops % 32).tolist()) == set(range(32)), "stop residues " + c["name"]
        assert bool((stops % 64 == 0).any()) and bool((stops % 64 == 63).any()), "no stop on a chunk boundary " + c["name"]
    if kind in ("sparse", "mixed"):
        n_untouched = sum(int((~walks[t]["use"].any(0)).sum()) for t, _, _ in tiles)
        assert n_untouched >= 0.3 * sum(r1 - r0 for _, r0, r1 in tiles), c["name"]
    if kind == "mixed":
        assert any(ref["tile_max"][t] < r1 - r0 for t, r0, r1 in tiles if r1 - r0 >= 128), "tile_max < total nowhere " + c["name"]
        deep = [t for t, r0, r1 in tiles if ref["tile_max"][t] >= 32]
        assert deep and all(bool((R.gather_image(ref["n_contrib"], t, c["H"], c["W"])[R.tile_pixels(t, c["H"], c["W"])[2]] == 0).any()) for t in deep)


def check_case(c, t):
    ref, err, amb = host_reference(c, t)
    assert amb == 0, "%d ambiguous (pixel, instance) pairs: replace the seed of %s" % (amb, c["name"])
    lens = t["lens"]
    tiles = R.tiles_of(t["ranges"], c["H"], c["W"])
    assert [r1 - r0 for _, r0, r1 in tiles] == [n for n in lens if n]
    assert c["tight"] or lens == LAYOUTS[c["layout"]]
    assert int(RG.bounds(t, dict(glue=False, deg=0, W=c["W"], H=c["H"]))[2].sum()) == 0, "an ambiguous Gaussian: replace the seed of " + c["name"]
    check_scene(c, ref, lens, tiles)
    if c["kind"] == "clamped":  # pairs at the clamp that are used
        rec, pl = t["records"], t["point_list"].long()
        n = 0
        for tl, r0, r1 in tiles:
            px, py, inside = R.tile_pixels(tl, c["H"], c["W"])
            wk = R._walk64(rec[pl[r0:r1]], px.double(), py.double(), inside)
            n += int((wk["use"] & (wk["alpha"] == R.ALPHA_MAX)).sum())
        assert n >= 8, "no clamped pair is used " + c["name"]


def make_cot(kind, c, g, given):
    """Image cotangents of a kind (tests/test_gpu_raster_gauss_f64._cot's kinds, per pixel); ``given``: with dL_ddepth and dL_dalpha."""
    H, W = c["H"], c["W"]
    x = torch.randn(5, H, W, generator=g)
    if kind == "same_sign":
        x = 1 + 0.3 * x
    elif kind == "sparse":
        x = torch.where(torch.rand(5, H, W, generator=g) < 0.2, x, torch.zeros_like(x))
    elif kind == "zero":
        x = torch.zeros_like(x)
    elif kind == "wide":
        x = x * torch.pow(10.0, -4.0 * torch.rand(1, H, W, generator=g))
    cot = {"color": x[:3].contiguous(), "depth": None, "alpha": None}
    if given:
        cot["depth"], cot["alpha"] = x[3].contiguous(), x[4].contiguous()
    return cot


INPUTS = ("means3D", "colors_precomp", "opacities", "cov3D_precomp")
WORST = {}  # case -> {what: worst err / bound} (tools/raster_comp_parity.py reads it after a run; nothing in the tests does)
VAC = {}    # case -> {array: largest vacuity share over the case's runs}


class Frame:
    """Device inputs of a case in front of NaN tails and a forward through the C ABI (``rasterize_forward``'s two calls)."""

    def __init__(self, c, t, arena=None, deterministic=False):
        self.c, self.t, self.N = c, t, t["N"]
        self.inp = {k: in_buf(t[k]) for k in INPUTS}
        self.st = GU.settings_for(camera(c), list(c["bg"]), 0, 1.0, debug=False)
        self.arena, self.det = arena, deterministic
        self.render()

    def render(self):
        from riggs_amd import rasterizer as RZ
        i = lambda k: self.inp[k][0]  # noqa: E731
        before = RZ.ORDERED_BACKWARD
        RZ.set_ordered_backward(self.det)
        try:
            res = RZ.rasterize_forward(self.st, i("means3D"), None, i("colors_precomp"), i("opacities"), None, None, i("cov3D_precomp"),
                                       arena=self.arena, tight_lists=self.c["tight"])
        finally:
            RZ.set_ordered_backward(before)
        torch.cuda.synchronize()
        self.color, self.radii, self.depth, self.alpha, self.s = res
        self.v = RZ.saved_views(self.s)
        v = self.v
        self.records = R.records_of(v["xyd"].cpu(), v["conic_o"].cpu(), v["rgb"].cpu())
        self.ranges, self.point_list = v["ranges"].cpu(), v["point_list"].cpu()
        return self

    def backward(self, cot, ordered):
        """riggs_raster_backward with NaN-prefilled outputs and the test's own zero-filled workspace -> (outputs, rows or None)."""
        s, N, lib = self.s, self.N, L.lib()
        base = int(lib.riggs_raster_backward_workspace_bytes(N))
        nbytes = int(lib.riggs_raster_backward_workspace_bytes_ordered(N, s.cap)) if ordered else base
        assert nbytes % 4 == 0 and base % 4 == 0 and (not ordered or nbytes >= base + s.cap * 40)
        ws = torch.zeros(nbytes // 4 + TAIL, dtype=torch.float32, device="cuda")
        ws[nbytes // 4:] = GU.SENT
        out = {k: out_buf(sh, fill=float("nan")) for k, sh in (("dL_dmeans3D", (N, 3)), ("dL_dmeans2D", (N, 3)), ("dL_dcolors_precomp", (N, 3)),
                                                               ("dL_dopacities", (N, 1)), ("dL_dcov3D", (N, 6)))}
        dev = lambda x: None if x is None else x.cuda().contiguous()  # noqa: E731
        gc, gd, ga = dev(cot["color"]), dev(cot["depth"]), dev(cot["alpha"])
        i = lambda k: self.inp[k][0].data_ptr()  # noqa: E731
        o = lambda k: out[k][0].data_ptr()  # noqa: E731
        cfg = s.cfg
        cfg.sparse_zero, cfg.deterministic = 0, 1 if ordered else 0
        L.check(lib.riggs_raster_backward(
            C.byref(cfg), i("means3D"), None, None, i("colors_precomp"), i("opacities"), None, None, i("cov3D_precomp"), None, None, None,
            s.radii.data_ptr(), s.geom.data_ptr(), s.binning.data_ptr(), s.cap, s.img.data_ptr(), s.counters.data_ptr(), gc.data_ptr(),
            L.ptr(gd), L.ptr(ga), ws.data_ptr(), o("dL_dmeans3D"), o("dL_dmeans2D"), None, o("dL_dcolors_precomp"), o("dL_dopacities"), None, None,
            o("dL_dcov3D"), None, None, L.stream_ptr()), "riggs_raster_backward")
        torch.cuda.synchronize()
        assert bool((ws[nbytes // 4:] == GU.SENT).all()), "write past the end of the workspace"
        for k, (view, buf) in out.items():
            assert bool(torch.isnan(buf[N:]).all()), "write past the end of " + k
            assert not bool(torch.isnan(view).any()), k + " is not fully written"
        for k, (_, buf) in self.inp.items():
            assert bool(torch.isnan(buf[N:]).all()), "input tail of %s changed" % k
        rows = None
        if ordered:
            Rn = self.v["R"]
            rows = ws[base // 4: base // 4 + Rn * 10].view(Rn, 10).cpu()
        else:
            assert bool((ws[:N * 12] == 0).all()), "the accumulators are not all zero again"
        return {k: v[0].cpu() for k, v in out.items()}, rows


def walk_history(f):
    """The walk-history words of the frame's view: one per tile (include/riggs_hip.h: RIGGS_BIN_WALK_HIST; 16 header words, word 1
    names the slot of the last frame, 128 slots of the tile count + 18 words rounded up to 16)."""
    s = f.s
    bo = (C.c_size_t * L.BIN_NFIELDS)()
    L.lib().riggs_raster_binning_layout(s.cap, s.N, s.H, s.W, bo)
    T = ((s.W + 15) // 16) * ((s.H + 15) // 16)
    slot_words = (T + 18 + 15) & ~15
    off = bo[L.BIN_WALK_HIST]
    words = s.binning[off:off + 4 * (16 + 128 * slot_words)].view(torch.int32).cpu().long() & 0xFFFFFFFF
    slot = int(words[1])
    return words[16 + slot * slot_words:16 + slot * slot_words + T]


def kernel_reference(c, f, cot=None):
    """Reference, bounds and ambiguity count from the KERNEL's records and lists; the designed lengths against its ranges."""
    t = f.t
    lens = t["lens"]  # (with tight lists: what the host's statement of the rule leaves of the designed lengths)
    tiles = R.tiles_of(f.ranges, c["H"], c["W"])
    got = f.ranges.long()
    assert (got[:, 1] - got[:, 0]).tolist() == list(lens), "the lists do not have the designed lengths"
    assert f.v["R"] == sum(lens) and f.N == sum(LAYOUTS[c["layout"]]) - STRADDLE
    hp, kp = t["point_list"].long(), f.point_list.long()  # (as sets per tile: the host's depths are a restatement's, an ulp may swap two)
    at = 0
    for n in lens:
        assert torch.equal(torch.sort(hp[at:at + n]).values, torch.sort(kp[at:at + n]).values), "a tile's list does not hold the host's Gaussians"
        at += n
    ref = R.reference(f.records, f.ranges, f.point_list, t["bg"], c["H"], c["W"], cot)
    err, val, amb = R.bounds(f.records, f.ranges, f.point_list, t["bg"], c["H"], c["W"], ref, cot)
    assert amb == 0, "%d ambiguous pairs on the kernel's records: replace the seed of %s" % (amb, c["name"])
    return ref, err, tiles


def _vac(c, k, ref, err):
    v = VAC.setdefault(c["name"], {})
    v[k] = max(v.get(k, 0.0), R.vacuity(ref, err))


def check_images(c, f, ref, err, tag):
    got = {"color": f.color.cpu(), "depth": f.depth.cpu()[0], "alpha": f.alpha.cpu()[0], "final_T": f.v["final_T"].cpu()}
    w = WORST.setdefault(c["name"], {})
    for k in R.IMG_KEYS:
        w["%s %s" % (k, tag)] = R.assert_within("%s %s %s" % (k, c["name"], tag), got[k].double(), ref[k], err[k], stats=GU.STATS)
        _vac(c, k, ref[k], err[k])
    assert torch.equal(f.v["n_contrib"].cpu().long(), ref["n_contrib"]), "n_contrib differs %s %s" % (c["name"], tag)


def check_rows(c, rows, ref, err, tiles, tag):
    w = WORST.setdefault(c["name"], {})
    w["rows " + tag] = R.assert_within("rows %s %s" % (c["name"], tag), rows.double(), ref["rows"], err["rows"], stats=GU.STATS)
    _vac(c, "rows", ref["rows"], err["rows"])
    for t, r0, r1 in tiles:  # behind the tile's walk limit nothing is walked: the memset's zeros, bit for bit
        lim = ref["tile_max"][t]
        assert bool((rows[r0 + lim:r1].view(torch.int32) == 0).all()), "a row behind the walk limit of tile %d is not +0 %s" % (t, tag)
        untouched = ~ref["walk"][t]["use"].any(0)
        assert bool((rows[r0:r1][untouched].view(torch.int32) == 0).all()), "the row of an untouched instance of tile %d is not +0 %s" % (t, tag)


def per_gaussian_reference(c, t, sums, sums_err, vis, given):
    """dL_dcov3D and dL_dmeans3D of the default mode: float64 autograd of the per-Gaussian stage contracted with the reference's
    per-Gaussian sums, and the stage's bounds with the sums' own bounds as the error of the record it reads."""
    rec, rec_err = sums.clone(), sums_err.clone()
    if not given:  # dL_ddepth NULL: the depth column is not accumulated
        rec[:, 9], rec_err[:, 9] = 0, 0
    cfg = dict(glue=False, deg=0, W=c["W"], H=c["H"])
    ref = RG.reference(t, cfg, rec, vis)["grads"]
    _, err, amb = RG.bounds(t, cfg, rec, vis, rec_err=rec_err)
    assert int(amb.sum()) == 0
    return ref, {k: err[k].reshape(ref[k].shape) for k in ("dL_dcov3D", "dL_dmeans3D")}


ALL_COTS = [(k, given) for k in COT_KINDS for given in (False, True)]


def cot_plan(c, form="lanes8"):
    """(cotangent kind, dL_ddepth / dL_dalpha given) per backward of a case behind a forward form.  The short layout: all ten.  The
    long layout (a second per backward on the host): ``random`` with everything given on every case, and the ten dealt out so that
    the long cases together run every one of them behind the 8-lane form (two each over the five kinds of scene) and again behind
    the 32-lane form (every third one over its three cases)."""
    if c["layout"] == "A":
        return list(ALL_COTS)
    if form == "lanes32":
        j = [x["name"] for x in WIDE].index(c["name"])
        part = ALL_COTS[j::len(WIDE)]
    else:
        i = KINDS.index(c["kind"])
        part = ALL_COTS[2 * i:2 * i + 2]
    return [("random", True)] + [x for x in part if x != ("random", True)]


def run_backwards(c, f, tag):
    g = torch.Generator().manual_seed(c["seed"] + 7)
    for kind, given in cot_plan(c, tag):
        cot = make_cot(kind, c, g, given)
        ref, err, tiles = kernel_reference(c, f, cot)
        what = "%s %s%s" % (tag, kind, "+dD+dA" if given else "")
        out_ordered, rows = f.backward(cot, ordered=True)
        check_rows(c, rows, ref, err, tiles, what)
        out_default, _ = f.backward(cot, ordered=False)
        # ---- per Gaussian, in the ordered gather's fixed order and in the atomics' free one: the six accumulator columns that reach
        # an output unchanged within the rows' bounds plus the sum's term, and the other four (conic A, B, C and depth) through the
        # per-Gaussian stage's own reference, which takes the sums as its record and their bounds as the record's error
        s, e = R.gaussian_sums(ref["rows"], err["rows"], f.point_list, f.N)
        assert bool((torch.bincount(f.point_list.long(), minlength=f.N)[f.t["straddlers"]] == 2).all())  # two rows meet in these sums
        gref, gerr = per_gaussian_reference(c, f.t, s, e, f.radii.cpu() > 0, given)
        w = WORST.setdefault(c["name"], {})
        for mode, out in (("ordered", out_ordered), ("default", out_default)):
            for k, got, cols in (("dL_dmeans2D", out["dL_dmeans2D"][:, :2], [0, 1]), ("dL_dopacities", out["dL_dopacities"], [5]),
                                 ("dL_dcolors_precomp", out["dL_dcolors_precomp"], [6, 7, 8])):
                w["%s %s %s" % (k, mode, what)] = R.assert_within("%s %s %s %s" % (k, c["name"], mode, what), got.double(), s[:, cols], e[:, cols],
                                                                  stats=GU.STATS)
            assert bool((out["dL_dmeans2D"][:, 2] == 0).all())
            for k in ("dL_dcov3D", "dL_dmeans3D"):
                w["%s %s %s" % (k, mode, what)] = R.assert_within("%s %s %s %s" % (k, c["name"], mode, what), out[k].double(), gref[k], gerr[k],
                                                                  stats=GU.STATS)


IDS = [c["name"] for c in GRID]


@pytest.mark.parametrize("c", GRID, ids=IDS)
def test_eight_lane_forward_and_the_backward_behind_it(c):
    """A fresh zero-filled arena (no walk history: every tile is composited by fw_block<8>), cfg.deterministic 0 and 1."""
    t = build(c)
    for det in (False, True):
        f = Frame(c, t, deterministic=det)
        assert int(f.v["fwd_ctr"][1]) == 0
        ref, err, tiles = kernel_reference(c, f)
        check_scene(c, ref, LAYOUTS[c["layout"]], tiles)
        check_images(c, f, ref, err, "lanes8 det%d" % det)
    run_backwards(c, f, "lanes8")


WIDE = [c for c in GRID if c["layout"] == "B" and c["kind"] in ("translucent", "opaque", "clamped")]


@pytest.mark.parametrize("c", WIDE, ids=[c["name"] for c in WIDE])
def test_wide_forward_and_the_backward_behind_it(c):
    """"fwd_wide_min" = 256 and two frames through one arena: the second composites with 32 lanes per pixel the tiles whose walk
    went 256 instances deep in the first.  WHICH tiles ran wide is inferred, not read: bit 31 of a tile's history word marks it only
    between the binning and the forward of the frame (the forward writes the tile's walk depth over it).  Read are the history
    words after the first frame — what the binning's choice, depth >= fwd_wide_min, is made from — and the count fwd_ctr[1] of the
    second; both must be what the design makes 256 deep."""
    from riggs_amd.rasterizer import RasterArena
    t = build(c)
    assert L.get_option("fwd_wide_min") == 4096
    L.set_option("fwd_wide_min", 256)
    try:
        arena = RasterArena(min_capacity=1024)
        f = Frame(c, t, arena=arena)
        assert int(f.v["fwd_ctr"][1]) == 0, "a fresh arena has no history: no wide tile"
        ref, err, tiles = kernel_reference(c, f)
        deep = [tl for tl, r0, r1 in tiles if ref["tile_max"][tl] >= 256]
        assert len(deep) >= 4, c["name"]
        hist = walk_history(f)
        for tl, r0, r1 in tiles:  # what the next frame's choice reads: how deep this frame walked every tile
            assert int(hist[tl]) == ref["tile_max"][tl], "the walk history of tile %d" % tl
        f.render()
        assert int(f.v["fwd_ctr"][1]) == len(deep) > 0, "the wide tiles are not the tiles the design makes 256 deep"
        ref, err, tiles = kernel_reference(c, f)
        check_images(c, f, ref, err, "lanes32")
        run_backwards(c, f, "lanes32")
    finally:
        L.set_option("fwd_wide_min", -1)
    assert L.get_option("fwd_wide_min") == 4096


def test_tight_lists():
    """cfg.tight_lists = 1 on a translucent scene in which 30 % of every list, at random positions, lies below 1/255: those instances
    get no list entry, the others move up — other positions, other groups of 8, other instances at the checkpoints.  ``build`` has
    asserted on the host that lists of 64 and more become shorter and that a long list loses an instance in front of its first
    chunk boundary; here the kernel's ranges and sorted list must be the host's (kernel_reference), and the reference is taken
    from the kernel's tight lists."""
    c = TIGHT
    t = build(c)
    f = Frame(c, t)
    lens = LAYOUTS[c["layout"]]
    got = (f.ranges.long()[:, 1] - f.ranges.long()[:, 0]).tolist()
    assert f.v["R"] < sum(lens), "cfg.tight_lists dropped nothing"
    assert sum(1 for n, m in zip(lens, got) if n >= 64 and m < n) >= 8 and max(got) >= 256
    ref, err, tiles = kernel_reference(c, f)
    check_images(c, f, ref, err, "tight")
    run_backwards(c, f, "tight")


RECOLOR = [BY_NAME["opaque-B-full"], BY_NAME["translucent-A-full"]]


@pytest.mark.parametrize("c", RECOLOR, ids=[c["name"] for c in RECOLOR])
def test_recolor_forward_and_backward(c):
    """riggs_raster_recolor_forward / _backward with a second colour set and another background: the image per pixel from the
    reference's weights alpha T over the instances in front of n_contrib, dL/dcolors per element with the free-order term."""
    from riggs_amd.rasterizer import recolor_backward, recolor_forward
    t = build(c)
    f = Frame(c, t)
    g = torch.Generator().manual_seed(c["seed"] + 99)
    colors = torch.rand(f.N, 3, generator=g)
    bg2 = torch.tensor([0.6, 0.05, 0.4])
    rec2 = f.records.clone()
    rec2[:, R.RR:R.BB + 1] = colors.double()
    cot = make_cot("random", c, g, False)
    ref = R.reference(rec2, f.ranges, f.point_list, bg2, c["H"], c["W"], cot)
    err, _, amb = R.bounds(rec2, f.ranges, f.point_list, bg2, c["H"], c["W"], ref, cot)
    assert amb == 0
    img = recolor_forward(f.s, colors.cuda(), bg2.cuda()).cpu()
    w = WORST.setdefault(c["name"], {})
    w["recolor image"] = R.assert_within("recolor image " + c["name"], img.double(), ref["color"], err["color"], stats=GU.STATS)
    gcol = recolor_backward(f.s, cot["color"].cuda()).cpu()
    s, e = R.gaussian_sums(ref["rows"], err["rows"], f.point_list, f.N)
    w["recolor dL_dcolors"] = R.assert_within("recolor dL_dcolors " + c["name"], gcol.double(), s[:, 6:9], e[:, 6:9], stats=GU.STATS)
