"""Float64 reference of the rasterizer's compositing stage (csrc/render.hip: fw_block<8>, fw_block_wide, render_bwd_kernel) and a
per-element bound for every output, per pixel and per tile instance.

The kernels are checked from the SAME fp32 numbers they read: the records of the geometry arena (x, y, depth | conic A, B, C,
opacity | r, g, b), the tile ``ranges`` and the sorted ``point_list``, cast exactly to float64.  What is left is compositing
arithmetic only.  Three pieces, as in tests/raster_gauss_ref.py:

``reference``   front-to-back per pixel in float64 torch: power = -0.5 (A dx^2 + C dy^2) - B dx dy, alpha = min(0.99, o exp(power)),
    the two skips (power > 0, alpha < 1/255), the stop rule T (1 - alpha) < 1e-4.  final_T is the transmittance IN FRONT of the
    instance that stops the pixel, n_contrib the position + 1 of the last USED instance.  The checkpoints are the exclusive state
    (T, C0, C1, C2, D) at every 64th instance.  Gradients are float64 AUTOGRAD with the decisions as constant masks; the records
    are gathered by point_list into one leaf per TILE INSTANCE, so autograd returns the backward's per-instance rows directly, in
    the row convention of render_bwd_kernel's final write: dL/d(NDC x) = dL/dx 0.5 W, dL/d(NDC y) = dL/dy 0.5 H, dL/dA, dL/dB,
    dL/dC (true partials of power), dL/d opacity, dL/d rgb, dL/d depth.  A clamped alpha still passes its gradient to opacity and
    conic (the kernel's and upstream's behaviour; tests/dense_splat.py's detach trick).  ``closed_form`` is the second opinion: the
    backward's prefix / suffix form with the background term, written once in float64 (host tests hold it to autograd at 1e-10).

``kernel_steps``   the kernels' own steps.  With ``F32`` it is the host restatement in float32, op by op: the forward in groups of 8
    (quad scans, the upper quad takes the lower quad's product), of 32 (shift-and-multiply scan over two rows of 16) or of 1, per-lane
    partial sums folded by a tree at the checkpoints and at the end, T advanced by the group's product; the backward in chunks of 64
    with the checkpoint-seeded product scan, the prefix-sum scan of w k, qb with the background term, the reciprocal of 1 - alpha,
    and the ten moments accumulated over four pixel parts of 64 pixels, in pairs of neighbouring pixels (the second one's dx is
    the first one's - 1), then folded.  ``order`` chooses grouping and fold order; ``fault`` plants one of FAULTS.  The ``Bounded``
    side is the error analysis of the same steps and runs through ``bounds`` (it takes the reference's decisions); its scans and
    folds are closed forms that hold for ANY bracketing, so one analysis covers the 8-lane form, the 32-lane form, the round's
    survivor lists of the wide block, the backward's re-evaluation from checkpoints and recolor.hip:

``bounds``   every quantity is a pair (v, e) of tests/raster_gauss_ref.py's ``Er``: v its float64 value, e a bound of |fp32 value - v|
    for any fp32 evaluation.  u = 2^-24.  Besides that module's rules (sum, product, quotient, constants):
        exp2 a:  v (2^e_a - 1) + 2 EXP_ULP u v + FLUSH   (v_exp_f32; EXP_ULP, FLUSH of tests/skin_ref.py); LOG2E carries its fp32 rounding
        rcp a:   e_a / (|a| (|a| - e_a)) + 2 RCP_ULP u / |a|        (v_rcp_f32: 1 ulp)
        product of m factors in any bracketing (the transmittance in front of an instance): relative error
                 expm1(sum_i e_i / (f_i - e_i) + (m - 1) u'), the factors 1.0 of skipped instances being exact
        sum of m non-zero terms in any order, also every prefix of it:  sum e_i + (m - 1) u sum (|t_i| + e_i)
    The amplification of an alpha error through 1 / (1 - alpha) (100 x at the clamp) and through long products is what these rules
    give; the cancellation total - prefix - own of the suffix carries the roundings of the TOTAL, not of the small difference.
    dx carries two roundings (the backward's second pixel of a pair), power the larger bound of the forward's and the backward's
    association.  No constant was tuned on kernel output.

Decisions.  power <= 0, alpha >= 1/255 and T (1 - alpha) < 1e-4 are re-made in fp32 by the kernels (forward: fast_exp; backward:
exp2(power LOG2E) on packed operands) and are not stored per pair.  A (pixel, instance) pair that the walk reaches is AMBIGUOUS when
one of the three lies within its own error bound of its threshold; the tests admit none, and then n_contrib must equal the
reference's exactly.  The forward's cull boxes and the backward's reject are conservative and decide nothing.

Pure torch on the CPU."""
import math

import numpy as np
import torch

from tests.raster_gauss_ref import F64, TINY, U, Bounded, Er, assert_within, vacuity, violations  # noqa: F401
from tests.skin_ref import EXP_ULP, FLUSH

RCP_ULP = 1.0
F32T = torch.float32
f32c = lambda x: float(np.float32(x))  # noqa: E731
ALPHA_MIN = float(np.float32(1.0) / np.float32(255.0))
ALPHA_MAX = f32c(0.99)
T_EPS = f32c(0.0001)
LOG2E = f32c(1.4426950408889634)
U1 = U / (1.0 - U)

IMG_KEYS = ("color", "depth", "alpha", "final_T")
FAULTS = ("stop_on_T", "thr_256", "clamp_blocks_grad", "final_T_behind", "n_contrib_counts_stop", "ckpt_late", "bg_dropped",
          "gA_1mT_dropped", "pair_dx", "depth_by_colour", "part_left_out", "wide_other_half", "ckpt_late_last")
# record columns of a tile instance's leaf
X, Y, Z, CA, CB, CC, OP, RR, GG, BB = range(10)


def records_of(xyd, conic_o, rgb):
    """(N, 10) float64 from the geometry arena's three float4 records (exact casts)."""
    return torch.cat([xyd[:, :3], conic_o[:, :4], rgb[:, :3]], 1).to(F64)


def tile_pixels(t, H, W):
    gx = (W + 15) // 16
    loc = torch.arange(256)
    px, py = (t % gx) * 16 + loc % 16, (t // gx) * 16 + loc // 16
    return px, py, (px < W) & (py < H)


def tiles_of(ranges, H, W):
    """[(tile, list start, list end)] of the non-empty tiles."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    rg = ranges.long().reshape(T, 2)
    return [(t, int(rg[t, 0]), int(rg[t, 1])) for t in range(T) if int(rg[t, 1]) > int(rg[t, 0])]


def scatter_image(dst, t, H, W, val):
    px, py, inside = tile_pixels(t, H, W)
    dst[..., py[inside], px[inside]] = val[..., inside]


def gather_image(img, t, H, W):
    """(..., 256) of a tile's pixels (0 outside the image)."""
    px, py, inside = tile_pixels(t, H, W)
    out = torch.zeros(img.shape[:-2] + (256,), dtype=img.dtype)
    out[..., inside] = img[..., py[inside], px[inside]]
    return out


# ------------------------------------------------------------------------------------------------ float64 reference
def _walk64(leaf, px, py, inside):
    """The differentiable float64 walk of one tile: per (pixel, instance) tensors and the decisions."""
    dx, dy = leaf[None, :, X] - px[:, None], leaf[None, :, Y] - py[:, None]
    pw = -0.5 * (leaf[None, :, CA] * dx * dx + leaf[None, :, CC] * dy * dy) - leaf[None, :, CB] * dx * dy
    G = torch.exp(pw)
    raw = leaf[None, :, OP] * G
    alpha = torch.where(raw > ALPHA_MAX, raw - (raw - ALPHA_MAX).detach(), raw)  # min(0.99, o G), the gradient still flowing
    cand = (pw.detach() <= 0) & (alpha.detach() >= ALPHA_MIN) & inside[:, None]
    om = torch.where(cand, 1 - alpha, torch.ones_like(alpha))
    cp = torch.cumprod(om, 1)
    Tex = torch.cat([torch.ones_like(cp[:, :1]), cp[:, :-1]], 1)
    stopc = cand & ((Tex * om).detach() < T_EPS)
    before = torch.cumsum(stopc.long(), 1) - stopc.long()
    reached = before == 0  # the walk gets to this instance
    use = cand & ~stopc & reached
    stopped = stopc.any(1)
    stop_pos = torch.where(stopped, stopc.long().argmax(1), torch.full_like(before[:, 0], -1))
    return dict(dx=dx, dy=dy, pw=pw, G=G, alpha=alpha, cand=cand, Tex=Tex, cp=cp, use=use, reached=reached, stopped=stopped, stop_pos=stop_pos)


def _final_T(wk, Tex, cp):
    idx = wk["stop_pos"].clamp_min(0)[:, None]
    return torch.where(wk["stopped"], Tex.gather(1, idx)[:, 0], cp[:, -1])


def reference(records, ranges, point_list, bg, H, W, cot=None):
    """``records`` (N, 10) float64 (records_of), ``ranges`` (T, 2), ``point_list`` (R,), ``bg`` (3,), ``cot``: None or a dict with
    ``color`` (3, H, W) and optionally ``depth`` / ``alpha`` (H, W).  Returns color (3, H, W), depth, alpha, final_T (H, W) float64,
    n_contrib (H, W) int64, ``ckpt`` {tile: (chunks, 5, 256)} with ``ckpt_valid`` {tile: (chunks, 256) bool} for lists of at least
    64, ``tile_max`` {tile: int}, ``walk`` {tile: decisions}, and with a cotangent ``rows`` (R, 10) and ``rows_closed`` (R, 10)."""
    bg = bg.to(F64)
    pl = point_list.long()
    out = {"color": bg[:, None, None].expand(3, H, W).clone(), "depth": torch.zeros(H, W, dtype=F64), "alpha": torch.zeros(H, W, dtype=F64),
           "final_T": torch.ones(H, W, dtype=F64), "n_contrib": torch.zeros(H, W, dtype=torch.int64), "ckpt": {}, "ckpt_valid": {}, "tile_max": {},
           "walk": {}}
    R = pl.shape[0]
    if cot is not None:
        out["rows"], out["rows_closed"] = torch.zeros(R, 10, dtype=F64), torch.zeros(R, 10, dtype=F64)
    for t, r0, r1 in tiles_of(ranges, H, W):
        px, py, inside = tile_pixels(t, H, W)
        pxd, pyd = px.to(F64), py.to(F64)
        leaf = records[pl[r0:r1]].clone().requires_grad_(cot is not None)
        wk = _walk64(leaf, pxd, pyd, inside)
        use, Tex, cp = wk["use"], wk["Tex"], wk["cp"]
        w = torch.where(use, wk["alpha"] * Tex, torch.zeros_like(Tex))
        Tfin = _final_T(wk, Tex, cp)
        col = w @ leaf[:, RR:BB + 1]
        dep, alp = w @ leaf[:, Z], w.sum(1)
        L = r1 - r0
        pos1 = torch.arange(1, L + 1)[None, :]
        n = torch.where(use, pos1, torch.zeros_like(pos1)).max(1).values
        scatter_image(out["color"], t, H, W, (col + Tfin[:, None] * bg[None]).detach().T)
        for k, v in (("depth", dep), ("alpha", alp), ("final_T", Tfin)):
            scatter_image(out[k], t, H, W, v.detach())
        scatter_image(out["n_contrib"], t, H, W, n)
        out["tile_max"][t] = int(n.max())
        out["walk"][t] = {k: wk[k] for k in ("use", "reached", "cand", "stopped", "stop_pos")}
        if L >= 64:
            at = torch.arange(0, L, 64)
            wd = w.detach()
            ex = lambda v: (torch.cumsum(wd * v[None], 1) - wd * v[None])[:, at]  # noqa: E731  (exclusive prefix at the chunk starts)
            ld = leaf.detach()
            out["ckpt"][t] = torch.stack([Tex.detach()[:, at], ex(ld[:, RR]), ex(ld[:, GG]), ex(ld[:, BB]), ex(ld[:, Z])], 0).permute(2, 0, 1)
            out["ckpt_valid"][t] = wk["reached"][:, at].T & inside[None]
        if cot is not None:
            gc, gd, ga = _cot_of_tile(cot, t, H, W)
            loss = (col * gc.T).sum() + (Tfin * (gc * bg[:, None]).sum(0)).sum() + (dep * gd).sum() + (alp * ga).sum()
            g, = torch.autograd.grad(loss, leaf, allow_unused=True)
            g = torch.zeros_like(leaf) if g is None else g
            out["rows"][r0:r1] = torch.stack([g[:, X] * (0.5 * W), g[:, Y] * (0.5 * H), g[:, CA], g[:, CB], g[:, CC], g[:, OP], g[:, RR], g[:, GG],
                                              g[:, BB], g[:, Z]], 1)
            out["rows_closed"][r0:r1] = closed_form(leaf.detach(), wk, w.detach(), Tfin.detach(), bg, gc, gd, ga, H, W)
    return out


def _cot_of_tile(cot, t, H, W):
    gc = gather_image(cot["color"].to(F64), t, H, W)
    z = torch.zeros(256, dtype=F64)
    gd = gather_image(cot["depth"].to(F64), t, H, W) if cot.get("depth") is not None else z
    ga = gather_image(cot["alpha"].to(F64), t, H, W) if cot.get("alpha") is not None else z
    return gc, gd, ga


def closed_form(leaf, wk, w, Tfin, bg, gc, gd, ga, H, W):
    """The backward's own form in float64: dL/dalpha_j = T_j k_j - (sum_{i > j} w_i k_i + T_final bg.g) / (1 - alpha_j), with
    k = g.c + g_D z + g_A; moments of q = dL/dalpha G over the tile's pixels."""
    use = wk["use"]
    k = gc.T @ leaf[:, RR:BB + 1].T + gd[:, None] * leaf[None, :, Z] + ga[:, None]
    wkk = w * k
    pre = torch.cumsum(wkk, 1) - wkk
    total = wkk.sum(1) + Tfin * (gc * bg[:, None]).sum(0)
    al = torch.where(use, wk["alpha"].detach(), torch.zeros_like(w))
    dLa = wk["Tex"].detach() * k - (total[:, None] - pre - wkk) / (1 - al)
    q = torch.where(use, dLa * wk["G"].detach(), torch.zeros_like(w))
    dx, dy = wk["dx"].detach(), wk["dy"].detach()
    o, A, B, C = leaf[:, OP], leaf[:, CA], leaf[:, CB], leaf[:, CC]
    mx, my = (q * dx).sum(0), (q * dy).sum(0)
    return torch.stack([-o * (A * mx + B * my) * (0.5 * W), -o * (C * my + B * mx) * (0.5 * H), -0.5 * o * (q * dx * dx).sum(0),
                        -o * (q * dx * dy).sum(0), -0.5 * o * (q * dy * dy).sum(0), q.sum(0), (w * gc[0][:, None]).sum(0),
                        (w * gc[1][:, None]).sum(0), (w * gc[2][:, None]).sum(0), (w * gd[:, None]).sum(0)], 1)


# ------------------------------------------------------------------------------------------------ the two arithmetics
class CompBounded(Bounded):
    """tests/raster_gauss_ref.py's error analysis with the compositing's own operations."""

    def twice(self, x):  # one more rounding of the same value
        return Er._rnd(x.v, x.e)

    def either(self, a, b):  # two associations of the same quantity: the first one's value, the larger bound
        return Er(a.v, torch.maximum(a.e, b.e + (a.v - b.v).abs()))

    def exp2(self, x):
        v = torch.exp2(x.v)
        return Er(v, v * torch.expm1(math.log(2.0) * x.e) + 2.0 * EXP_ULP * U * v + FLUSH)

    def rcp(self, x):
        v = 1.0 / x.v
        room = (x.v.abs() - x.e).clamp_min(1e-300)
        return Er(v, x.e / (x.v.abs() * room) + 2.0 * RCP_ULP * U * v.abs())

    def minc(self, x, c):  # (1-Lipschitz; where every evaluation lies above the constant the result IS the constant)
        return Er(x.v.clamp_max(c), torch.where(x.v - x.e >= c, torch.zeros_like(x.e), x.e))

    def mask(self, m, x):
        return Er(torch.where(m, x.v, torch.zeros_like(x.v)), torch.where(m, x.e, torch.zeros_like(x.e)))

    def excl_prod(self, f, counted):
        """Exclusive running product along dim 1 of the factors ``f`` (1.0 exactly where not ``counted``), in any bracketing."""
        cp = torch.cumprod(f.v, 1)
        v = torch.cat([torch.ones_like(cp[:, :1]), cp[:, :-1]], 1)
        rel = torch.where(counted, f.e / (f.v - f.e).clamp_min(1e-300), torch.zeros_like(f.e))
        m = torch.cumsum(counted.to(F64), 1)
        rho = torch.cumsum(rel, 1) + (m - 1).clamp_min(0) * U1
        rho = torch.cat([torch.zeros_like(rho[:, :1]), rho[:, :-1]], 1)
        return Er(v, v * torch.expm1(rho))

    @staticmethod
    def _sum_err(t, dim, excl):
        nz = ((t.v.abs() + t.e) > 0).to(F64)
        m, se, sa = torch.cumsum(nz, dim), torch.cumsum(t.e, dim), torch.cumsum(t.v.abs() + t.e, dim)
        e = se + (m - 1).clamp_min(0) * U * sa + TINY * (sa > 0)
        v = torch.cumsum(t.v, dim)
        if excl:
            v, e = v - t.v, e.roll(1, dim)
            e.select(dim, 0).zero_()
        return v, e

    def prefix(self, t, dim=1):
        """Exclusive prefix sums of the terms along ``dim``, the terms in front of each element added in any order."""
        return Er(*self._sum_err(t, dim, True))

    def total(self, t, dim):
        v, e = self._sum_err(t, dim, False)
        return Er(v.select(dim, -1), e.select(dim, -1))


def _pair_math(A, rec, pxd, pyd):
    """power, G = exp2(power LOG2E), o G and alpha of every (pixel, instance) pair over the arithmetic ``A`` (the Bounded one)."""
    c = lambda j: A.inp(rec[None, :, j])  # noqa: E731
    x, y, a, b, cc, o = c(X), c(Y), c(CA), c(CB), c(CC), c(OP)
    dx = A.twice(x - A.inp(pxd[:, None]))
    dy = y - A.inp(pyd[:, None])
    quad = -0.5 * (a * dx * dx + cc * dy * dy)
    pw = A.either(quad - b * dx * dy, quad - (b * dy) * dx)
    G = A.exp2(pw * A.const(1.4426950408889634))
    raw = o * G
    return dx, dy, pw, G, raw, A.minc(raw, ALPHA_MAX)


def bounds(records, ranges, point_list, bg, H, W, ref, cot=None):
    """{array: per-element bound} for ``reference``'s outputs ``ref`` (whose decisions it takes): color (3, H, W), depth, alpha,
    final_T (H, W), and with a cotangent ``rows`` (R, 10) and ``ckpt`` {tile: (chunks, 5, 256)}, the checkpoints' own prefix bounds; ``values`` {array: the float64 value of the kernel's own steps} (a third
    opinion); ``ambiguous``: the number of reached (pixel, instance) pairs with a decision within its error of its threshold."""
    A = CompBounded()
    bgf = bg.to(F64)
    pl = point_list.long()
    err = {"color": torch.zeros(3, H, W, dtype=F64), "depth": torch.zeros(H, W, dtype=F64), "alpha": torch.zeros(H, W, dtype=F64),
           "final_T": torch.zeros(H, W, dtype=F64)}
    val = {}
    if cot is not None:
        err["rows"], val["rows"] = torch.zeros(pl.shape[0], 10, dtype=F64), torch.zeros(pl.shape[0], 10, dtype=F64)
    amb = 0
    with torch.no_grad():
        for t, r0, r1 in tiles_of(ranges, H, W):
            px, py, inside = tile_pixels(t, H, W)
            rec = records[pl[r0:r1]]
            L = r1 - r0
            wk = ref["walk"][t]
            use, reached = wk["use"], wk["reached"] & inside[:, None]
            dx, dy, pw, G, raw, alpha = _pair_math(A, rec, px.to(F64), py.to(F64))
            al = A.mask(use, alpha)
            om = 1.0 - al
            om = Er(om.v, torch.where(use, om.e, torch.zeros_like(om.e)))  # (1 - 0 is exact)
            Tl = A.excl_prod(om, use)
            # ---- ambiguous decisions among the pairs the walk reaches
            a_pw = (pw.v <= 0) & (pw.v + pw.e > 0) | (pw.v > 0) & (pw.v - pw.e <= 0)
            a_al = (pw.v <= 0) & ((alpha.v - ALPHA_MIN).abs() <= alpha.e)
            test = Tl * (1.0 - alpha)
            a_T = wk["cand"] & ((test.v - T_EPS).abs() <= test.e)
            amb += int((reached & (a_pw | a_al | a_T)).sum())
            # ---- forward sums
            w = A.mask(use, al * Tl)
            cols = [A.inp(rec[None, :, j]) for j in (RR, GG, BB, Z)]
            tw = [w * c for c in cols]
            acc = [A.total(x, 1) for x in tw]
            asum = A.total(w, 1)
            idx = wk["stop_pos"].clamp_min(0)[:, None]
            Tend = Tl * om
            Tn = Er(torch.where(wk["stopped"], Tl.v.gather(1, idx)[:, 0], Tend.v[:, -1]), torch.where(wk["stopped"], Tl.e.gather(1, idx)[:, 0], Tend.e[:, -1]))
            colr = [acc[c] + Tn * A.inp(bgf[c]) for c in range(3)]
            scatter_image(err["color"], t, H, W, torch.stack([x.e for x in colr], 0))
            for k, x in (("depth", acc[3]), ("alpha", asum), ("final_T", Tn)):
                scatter_image(err[k], t, H, W, x.e)
            if cot is None:
                continue
            # ---- backward: chunks of 64 seeded with the forward's checkpoints
            gc, gd, ga = _cot_of_tile(cot, t, H, W)
            g = [A.inp(x[:, None]) for x in (gc[0], gc[1], gc[2], gd, ga)]
            k = A.fsum([g[0] * cols[0], g[1] * cols[1], g[2] * cols[2], g[3] * cols[3], Er(g[4].v + torch.zeros_like(w.v))])
            wkk = w * k
            pad = (-L) % 64
            P2 = lambda x: torch.cat([x, torch.zeros(256, pad, dtype=F64)], 1).reshape(256, -1, 64)  # noqa: E731
            E3 = lambda x: Er(P2(x.v), P2(x.e))  # noqa: E731
            S = [A.prefix(x, 1) for x in tw]                       # any-order prefixes: the checkpoint sums at the chunk starts
            at = torch.arange(0, L, 64)
            Sk = [Er(x.v[:, at], x.e[:, at]) for x in S]
            Ts = Er(Tl.v[:, at], Tl.e[:, at])
            err.setdefault("ckpt", {})[t] = torch.stack([Ts.e] + [x.e for x in Sk], 0).permute(2, 0, 1)  # (chunks, 5, 256)
            pre0 = A.fsum([g[0] * Sk[0], g[1] * Sk[1], g[2] * Sk[2], g[3] * Sk[3], g[4] * (1.0 - Ts)])
            scan = A.prefix(E3(wkk), 2)
            pre = Er(pre0.v[:, :, None], pre0.e[:, :, None]) + scan
            pre = Er(pre.v.reshape(256, -1)[:, :L], pre.e.reshape(256, -1)[:, :L])
            Tn1 = Er(Tn.v[:, None], Tn.e[:, None])
            a1 = [Er(x.v[:, None], x.e[:, None]) for x in acc]
            qb = A.fsum([g[0] * a1[0], g[1] * a1[1], g[2] * a1[2], g[3] * a1[3], g[4] * (1.0 - Tn1)]) + \
                Tn1 * A.fsum([A.inp(bgf[0]) * g[0], A.inp(bgf[1]) * g[1], A.inp(bgf[2]) * g[2]])
            dLa = Tl * k - (qb - pre - wkk) * A.rcp(om)
            q = A.mask(use, dLa * G)
            qx, qy = q * dx, q * dy
            mom = [qx, qy, qx * dx, qx * dy, qy * dy, q, w * g[0], w * g[1], w * g[2], w * g[3]]
            m = [A.total(x, 0) for x in mom]
            c1 = lambda j: A.inp(rec[:, j])  # noqa: E731
            o, ca, cb, cc = c1(OP), c1(CA), c1(CB), c1(CC)
            a_mx, a_my = -(o * (ca * m[0] + cb * m[1])), -(o * (cc * m[1] + cb * m[0]))
            rows = [a_mx * f32c(0.5 * W), a_my * f32c(0.5 * H), -0.5 * (m[2] * o), -(m[3] * o), -0.5 * (m[4] * o)] + m[5:]
            err["rows"][r0:r1] = torch.stack([x.e for x in rows], 1)
            val["rows"][r0:r1] = torch.stack([x.v for x in rows], 1)
    return err, val, amb


def gaussian_sums(rows, rows_err, point_list, N):
    """Per Gaussian: the float64 sum of its instances' rows, and its bound — the rows' bounds plus the free-order term
    (n_tiles - 1) u sum |row| of the atomics."""
    pl = point_list.long()
    s = torch.zeros(N, 10, dtype=F64).index_add_(0, pl, rows)
    e = torch.zeros(N, 10, dtype=F64).index_add_(0, pl, rows_err)
    sa = torch.zeros(N, 10, dtype=F64).index_add_(0, pl, rows.abs() + rows_err)
    n = torch.zeros(N, dtype=F64).index_add_(0, pl, torch.ones(pl.shape[0], dtype=F64))
    return s, e + (n - 1).clamp_min(0)[:, None] * U * sa


# ------------------------------------------------------------------------------------------------ the float32 restatement
def _tree(x):
    """Fold of the last dim by the lanes' xor tree: (l0 + l1) + (l2 + l3), ..."""
    while x.shape[-1] > 1:
        x = x.reshape(x.shape[:-1] + (x.shape[-1] // 2, 2))
        x = x[..., 0] + x[..., 1]
    return x[..., 0]


def _shift(x, s, ident):
    return torch.cat([torch.full_like(x[..., :s], ident), x[..., :-s]], -1)


def _hs_scan(x, mul):
    """The DPP scan, inclusive: row_shr 1, 2, 4, 8 inside rows of 16 lanes, row_bcast:15 (rows 1 and 3 take the last lane of the row
    in front), row_bcast:31 (rows 2 and 3 take lane 31)."""
    n = x.shape[-1]
    r = min(16, n)
    op = (lambda a, b: a * b) if mul else (lambda a, b: a + b)
    y = x.reshape(x.shape[:-1] + (n // r, r))
    s = 1
    while s < r:
        y = op(y, _shift(y, s, 1.0 if mul else 0.0))
        s *= 2
    rows = [y[..., j, :] for j in range(n // r)]
    if len(rows) >= 2:
        rows[1] = op(rows[1], rows[0][..., -1:])
    if len(rows) == 4:
        rows[3] = op(rows[3], rows[2][..., -1:])
        c = rows[1][..., -1:]
        rows[2], rows[3] = op(rows[2], c), op(rows[3], c)
    return torch.stack(rows, -2).reshape(x.shape)


def _excl(x, mul, seq):
    """Exclusive scan along the last dim in float32: the DPP form or lane after lane."""
    if seq:
        out = [torch.full_like(x[..., 0], 1.0 if mul else 0.0)]
        for j in range(x.shape[-1] - 1):
            out.append(out[-1] * x[..., j] if mul else out[-1] + x[..., j])
        return torch.stack(out, -1)
    return _shift(_hs_scan(x, mul), 1, 1.0 if mul else 0.0)


class F32:
    """The float32 restatement.  ``order`` 0: the kernels' forms (forward groups of 8, DPP scans, the backward's parts and pairs);
    1: forward groups of 32, lane-after-lane scans in the backward, its pixels summed in reverse order; 2: one instance per step,
    DPP scans, the pixels summed by torch.sum."""
    name = "f32"

    def __init__(self, order=0):
        self.order = order
        self.group = (8, 32, 1)[order]


def _fw32(A, rec, px, py, inside, bg, fault):
    """One tile's forward in float32 -> per-pixel outputs, checkpoints (chunks, 5, 256) and their validity."""
    f = lambda x: x.to(F32T)  # noqa: E731
    G_ = A.group
    L = rec.shape[0]
    pad = (-L) % max(G_, 1)
    r = f(torch.cat([rec, torch.zeros(pad, 10, dtype=rec.dtype)], 0))
    Lp = L + pad
    dx, dy = r[None, :, X] - f(px)[:, None], r[None, :, Y] - f(py)[:, None]
    pw = -0.5 * (r[None, :, CA] * dx * dx + r[None, :, CC] * dy * dy) - r[None, :, CB] * dx * dy
    alpha = torch.clamp_max(r[None, :, OP] * torch.exp2(pw * LOG2E), ALPHA_MAX)
    thr = f32c(1.0 / 256.0) if fault == "thr_256" else ALPHA_MIN
    cand = (pw <= 0) & (alpha >= thr) & inside[:, None] & (torch.arange(Lp) < L)[None]
    one = torch.ones(256, dtype=F32T)
    T, done, Tstop, last = one.clone(), ~inside, -one, torch.zeros(256, dtype=torch.int64)
    part = torch.zeros(256, G_, 5, dtype=F32T)
    Tj_all, wt_all = torch.ones(256, Lp, dtype=F32T), torch.zeros(256, Lp, dtype=F32T)
    cks, ckv = [], []
    vals = torch.stack([r[:, RR], r[:, GG], r[:, BB], r[:, Z], torch.ones(Lp, dtype=F32T)], 1)
    for g0 in range(0, Lp, G_):
        if g0 % 64 == 0 and g0 < L:
            fold = _tree(part[:, :, :4].transpose(1, 2))
            cks.append(torch.cat([T[:, None], fold], 1))
            ckv.append(~done)
        sl = slice(g0, g0 + G_)
        valid = cand[:, sl] & ~done[:, None]
        a = alpha[:, sl]
        om = torch.where(valid, 1.0 - a, torch.ones_like(a))
        if G_ == 8:
            q = om.reshape(256, 2, 4)
            Eq = torch.stack([torch.ones_like(q[..., 0]), q[..., 0], q[..., 1] * q[..., 0], q[..., 2] * q[..., 1] * q[..., 0]], -1)
            Pq = Eq[..., 3] * q[..., 3]
            E = torch.cat([Eq[:, 0], Eq[:, 1] * Pq[:, :1]], 1)
            prod = E[:, 7] * om[:, 7]
        elif G_ == 32:
            inc = _hs_scan(om, True)
            E, prod = _shift(inc, 1, 1.0), inc[:, -1]
            if fault == "wide_other_half":
                prod = prod.reshape(128, 2).flip(1).reshape(256)  # the product of the wave's other pixel
        else:
            E, prod = torch.ones_like(om), om[:, 0]
        Tj = T[:, None] * E
        test = Tj if fault == "stop_on_T" else Tj * om
        sc = valid & (test < T_EPS)
        fsb = (torch.cumsum(sc.long(), 1) - sc.long()) > 0
        use = valid & ~sc & ~fsb
        wt = torch.where(use, a * Tj, torch.zeros_like(a))
        part = part + vals[None, sl, :] * wt[:, :, None]
        pos1 = torch.arange(g0 + 1, g0 + G_ + 1)[None]
        here = sc & ~fsb
        counted = use | here if fault == "n_contrib_counts_stop" else use
        last = torch.where(counted.any(1), torch.where(counted, pos1, torch.zeros_like(pos1)).max(1).values, last)
        ts = (test if fault == "final_T_behind" else Tj).gather(1, here.long().argmax(1)[:, None])[:, 0]
        Tstop = torch.where(here.any(1), ts, Tstop)
        nostop = ~sc.any(1)
        T = torch.where(nostop & ~done, T * prod, T)
        done = done | ~nostop
        Tj_all[:, sl], wt_all[:, sl] = Tj, wt
    k = _tree(part.transpose(1, 2))
    Tfin = torch.where(Tstop >= 0, Tstop, T)
    o = {"acc": k[:, :4], "alpha": k[:, 4], "final_T": Tfin, "n": last, "color": k[:, :3] + Tfin[:, None] * f(bg)[None], "depth": k[:, 3]}
    if cks:
        ck, cv = torch.stack(cks, 0).transpose(1, 2).clone(), torch.stack(ckv, 0)
        if fault in ("ckpt_late", "ckpt_late_last"):  # the state one instance late: behind instance 64 k instead of in front of it
            js = list(range(ck.shape[0]))
            if fault == "ckpt_late_last":  # ONE chunk of the scene: the last one, of a list of more than ten, whose first instance is used
                js = [j for j in js if ck.shape[0] > 10 and 64 * j + 1 < L and bool((wt_all[:, 64 * j] != 0).any())][-1:]
            for j in js:
                p = 64 * j
                if p + 1 < L:
                    ck[j, 0] = Tj_all[:, p + 1]
                    ck[j, 1:] = ck[j, 1:] + (vals[p, :4][:, None] * wt_all[None, :, p])
        o["ckpt"], o["ckpt_valid"] = ck, cv
    return o


def _bw32(A, rec, px, py, inside, bg, fw, gc, gd, ga, H, W, fault):
    """One tile's backward in float32 from the forward ``fw`` of the same arithmetic -> rows (L, 10), exactly 0 where untouched."""
    f = lambda x: x.to(F32T)  # noqa: E731
    L = rec.shape[0]
    n = fw["n"] * inside.long()
    limit = min(L, int(n.max()))
    rows = torch.zeros(L, 10, dtype=F32T)
    g0, g1, g2, gD, gA = f(gc[0]), f(gc[1]), f(gc[2]), f(gd), f(ga)
    b = f(bg)
    Tn, acc = fw["final_T"], fw["acc"]
    tail = Tn * (b[0] * g0 + b[1] * g1 + b[2] * g2)
    first = g0 * acc[:, 0] + g1 * acc[:, 1] + g2 * acc[:, 2] + gD * acc[:, 3]
    if fault != "gA_1mT_dropped":
        first = first + gA * (1.0 - Tn)
    qb_all = first if fault == "bg_dropped" else first + tail
    seq = A.order == 1
    pxA = f(px - (px % 2))  # the first pixel of the pair
    odd = (px % 2 == 1)[:, None]
    ddx, ddy = f32c(0.5 * W), f32c(0.5 * H)
    for k in range((limit + 63) // 64):
        pos0 = 64 * k
        cnt = min(64, limit - pos0)
        r = f(torch.cat([rec[pos0:pos0 + cnt], torch.zeros(64 - cnt, 10, dtype=rec.dtype)], 0))
        active = (torch.arange(64) < cnt)[None]
        live = n > pos0
        ck = fw["ckpt"][k] if "ckpt" in fw else torch.cat([torch.ones(1, 256), torch.zeros(4, 256)], 0).to(F32T)
        Ts = torch.where(live, ck[0], torch.ones_like(ck[0]))
        pre0 = g0 * ck[1] + g1 * ck[2] + g2 * ck[3] + gD * ck[4] + gA * (1.0 - ck[0])
        z = torch.zeros(256, dtype=F32T)
        pre0, qb = torch.where(live, pre0, z), torch.where(live, qb_all, z)
        s0, s1, s2, sD, sA = (torch.where(live, x, z) for x in (g0, g1, g2, gD, gA))
        dxA = r[None, :, X] - pxA[:, None]
        dx = dxA if fault == "pair_dx" else torch.where(odd, dxA - 1.0, dxA)
        dy = r[None, :, Y] - f(py)[:, None]
        cyy, cody = r[None, :, CC] * dy * dy, r[None, :, CB] * dy
        pw = -0.5 * (r[None, :, CA] * dx * dx + cyy) - cody * dx
        Gr = torch.exp2(pw * LOG2E)
        ar = r[None, :, OP] * Gr
        al_ = torch.clamp_max(ar, ALPHA_MAX)
        v = active & ((pos0 + torch.arange(64))[None] < n[:, None]) & (pw <= 0) & (al_ >= ALPHA_MIN)
        zz = torch.zeros_like(al_)
        al, Gm = torch.where(v, al_, zz), torch.where(v, Gr, zz)
        if fault == "clamp_blocks_grad":
            Gm = torch.where(ar > ALPHA_MAX, zz, Gm)
        om = 1.0 - al
        Tl = Ts[:, None] * _excl(om, True, seq)
        w = al * Tl
        kk = s0[:, None] * r[None, :, RR] + s1[:, None] * r[None, :, GG] + s2[:, None] * r[None, :, BB] + sD[:, None] * r[None, :, Z] + sA[:, None]
        wkk = w * kk
        pre = pre0[:, None] + _excl(wkk, False, seq)
        dLa = Tl * kk - (qb[:, None] - pre - wkk) * (1.0 / om)
        q = dLa * Gm
        qx, qy = q * dx, q * dy
        dcol = s2 if fault == "depth_by_colour" else sD
        mom = torch.stack([qx, qy, qx * dx, qx * dy, qy * dy, q, w * s0[:, None], w * s1[:, None], w * s2[:, None], w * dcol[:, None]], -1)
        if A.order == 0:  # parts = rows part, part + 4, ...; pairs of neighbouring pixels, (A, B) accumulators, then the folds
            x = mom.reshape(4, 4, 8, 2, 64, 10).permute(1, 0, 2, 3, 4, 5).reshape(4, 32, 2, 64, 10)
            accp = torch.zeros(4, 2, 64, 10, dtype=F32T)
            for j in range(32):
                accp = accp + x[:, j]
            prt = accp[:, 0] + accp[:, 1]
            m = prt[0]
            for j in range(1, 3 if fault == "part_left_out" else 4):
                m = m + prt[j]
        elif A.order == 1:
            m = torch.zeros(64, 10, dtype=F32T)
            for p in range(255, -1, -1):
                if bool(live[p]):
                    m = m + mom[p]
        else:
            m = mom.sum(0)
        o, ca, cb, cc = r[:, OP], r[:, CA], r[:, CB], r[:, CC]
        a_mx, a_my = -o * (ca * m[:, 0] + cb * m[:, 1]), -o * (cc * m[:, 1] + cb * m[:, 0])
        row = torch.stack([a_mx * ddx, a_my * ddy, -0.5 * (m[:, 2] * o), -(m[:, 3] * o), -0.5 * (m[:, 4] * o), m[:, 5], m[:, 6], m[:, 7], m[:, 8], m[:, 9]], 1)
        touched = v.any(0)
        rows[pos0:pos0 + cnt] = torch.where(touched[:cnt, None], row[:cnt], torch.zeros_like(row[:cnt]))
    return rows


def kernel_steps(A, records, ranges, point_list, bg, H, W, cot=None, fault=None):
    """The kernels' steps over the arithmetic ``A``.  ``F32``: the float32 restatement -> images (float32), n_contrib, and with a
    cotangent the rows (R, 10).  ``CompBounded``: see ``bounds`` (which needs the reference's decisions)."""
    assert fault is None or fault in FAULTS
    assert isinstance(A, F32), "the Bounded arithmetic runs through bounds(): it takes the reference's decisions"
    pl = point_list.long()
    out = {"color": bg.to(F32T)[:, None, None].expand(3, H, W).clone(), "depth": torch.zeros(H, W), "alpha": torch.zeros(H, W),
           "final_T": torch.ones(H, W), "n_contrib": torch.zeros(H, W, dtype=torch.int64), "ckpt": {}}
    if cot is not None:
        out["rows"] = torch.zeros(pl.shape[0], 10)
    with torch.no_grad():
        for t, r0, r1 in tiles_of(ranges, H, W):
            px, py, inside = tile_pixels(t, H, W)
            rec = records[pl[r0:r1]]
            fw = _fw32(A, rec, px, py, inside, bg, fault)
            scatter_image(out["color"], t, H, W, fw["color"].T)
            for k in ("depth", "alpha", "final_T"):
                scatter_image(out[k], t, H, W, fw[k])
            scatter_image(out["n_contrib"], t, H, W, fw["n"])
            if "ckpt" in fw:
                out["ckpt"][t] = (fw["ckpt"], fw["ckpt_valid"])
            if cot is not None:
                gc, gd, ga = _cot_of_tile(cot, t, H, W)
                out["rows"][r0:r1] = _bw32(A, rec, px, py, inside, bg, fw, gc, gd, ga, H, W, fault)
    return out
