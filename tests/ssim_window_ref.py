"""Float64 references, per-pixel rounding bounds and a numpy float32 restatement (with planted faults) of the two kernels that share
the 11-tap window body csrc/ssim_window.h: the image loss (csrc/loss.hip) and the evaluation report (csrc/metrics.hip).

TEST INFRASTRUCTURE ONLY (tests/test_ssim_window_ref_cpu.py, tests/test_gpu_ssim_window_f64.py, tools/ssim_window_parity.py).

**References.**  Float64 throughout, with the kernel's own taps: ``win_f32`` is ``fill_window_f32`` restated (float32 exps, serial
float32 sum, float32 divide), ``win_f64`` is ``fill_window_f64``; the 2-D window is the exact product w_i w_j (the separable
application in float64).  The trainer's window is the float32 rounding of that product: at most one rounding per tap away
(``window_distance``), i.e. 1 u of G*|v| against the trainer's definition; oracle/loss_ref.py (which uses that rounded outer product,
numpy's pairwise float32 sum and the double constants) stays the independent second opinion.

**Bounds** (u = 2^-24, first order; every final bound carries the factor ``SLACK`` = 1 + 2^-10 for the second-order terms, which are
below 100 u of the first-order ones).  ``E`` carries (value, bound, magnitude, roundings): the running error of one expression,
operation by operation:

* a rounded result r has |fl(r) - r| <= u |r|; the computed operands are within their own bounds, so the rounding is charged on
  |r| + bound;
* a + b: e_a + e_b;  a b: |a| e_b + |b| e_a + e_a e_b;  a / b: (e_a + |a / b| e_b) / (|b| - e_b), which needs e_b < |b| / 2
  (``Denominator``: raised per case on the host when it does not hold; both divisions of the loss and of the metrics are by sums
  that contain C2 = 9e-4 / C1 = 1e-4, and it held on every case of the grid).
* loss.hip and metrics.hip are built with -ffp-contract=fast: the compiler may fuse any product into the add or subtract that
  follows.  A fused operation DROPS the product's rounding and changes nothing else, so a bound that charges every rounding of the
  unfused form holds for every mix of fused and unfused operations (also where one product is used twice, fused once: each use is
  within the same bound).  Nothing here assumes either form; the restatement is accepted in both.
* The window (``sw_taps4`` / ``sw_tap_moments``): each separable pass is 11 serial FMAs from 0 with taps ascending, i.e. at most 11
  roundings on a term, 22 over both passes: 22 u G*|v|.  The products x x, y y, x y are formed (one rounding) before the taps:
  23 u G*|x y|.  The taps are non-negative, so G*|v| is the sum of the absolute values of the 121 terms.
* Forward epilogue of ``l1_ssim_forward_kernel``: mu1_sq, mu2_sq, mu12, sigma1, sigma2, sigma12, A, B, Cc, D, Cc D, inv = 1 / (Cc D)
  (correctly rounded: -fhip-fp32-correctly-rounded-divide-sqrt), ssim = (A B) inv, d/dmu1 = ((2 m2)(B - A)) inv - (((ssim 2) m1)
  (D - Cc)) inv, d/dE[x^2] = -ssim / D, d/dE[xy] = (2 A) inv, in the order the source has them (products by 2 are exact, but are
  charged).  |x - y|: one rounding.
* Per-workgroup partials: the tile's per-pixel bounds summed, plus the sum's own 13 roundings (4 serial adds per thread, the six
  steps of ``wave_sum``, three levels over the eight waves) on the sum of |value| + bound.
* ``out3`` from the kernel's own partials: their float64 sum times 1 / n, one cast (u).  out3[2] = (1 - lambda) l1 + lambda (1 - ssim)
  from out3[0], out3[1]: five roundings, two on each of the two terms a, b and one on their sum, hence <= 3 u (|a| + |b|).
* Backward epilogue of ``l1_ssim_backward_kernel``: the three convolutions at 22 u G*|map| each, inv_n = 1 / float(C H W) one
  rounding, gl = g_l1 + (1 - lambda) g_loss and gs = g_ssim - lambda g_loss as the kernel forms them in float32 (charged even where
  g_loss is NULL and they are exact), then ((gl sgn) inv_n) + ((gs inv_n) ((cv_a + (2 x) cv_b) + y cv_c)).
  The STAGE bound takes the maps the kernel itself wrote as exact inputs; the END-TO-END bound adds the maps' own bounds pushed
  through the window, G*e_a + |2 x| G*e_b + |y| G*e_c.
* Metrics level (``metrics_level_kernel``), a separate derivation of the SHIFTED form: x - 0.5 is exact for 0.25 <= x <= 2
  (Sterbenz / a common exponent grid) and one rounding elsewhere; the five moments are of the shifted values (22 u / 23 u as above
  on top of the shifted values' own error); sigma = E - m m; mu = m + 0.5 is one rounding; cs = (2 s12 + C2) / (s1 + s2 + C2);
  ssim = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) cs.  The reference is the same shifted form in float64: with taps that sum to
  1 - 1.4e-9 the shifted and the unshifted definitions differ by up to ~1e-6 of cs where the variances vanish against C2, which is
  the means' test's subject
  (tests/test_gpu_metrics.py), not a rounding of the kernel.  The partials are float64 sums of float32 values: the per-pixel
  bounds summed (+ 1e-13 relative for the float64 adds).
* Pools: serial float32 adds and one correctly rounded division, all of which numpy float32 does identically: compared bit for bit
  with ``restate_pool``, and within 4 u (three adds and the division at k = 2; (k^2 - 1) + 1 in general, k^2 u is used) of float64.
* ``levels`` / ``out``: float64 arithmetic on the kernel's own partials, one cast; 2 u is allowed (the cast + libm's pow / log10).

**Vacuity** of an array on a case: the share of its non-zero-reference elements whose bound reaches |reference|.  At most
``VACUITY_CAP`` on the scored families, decided on the host.  ``dark`` is counted over the masked-in region plus a 5-pixel rim
(the pixels whose window meets the object): beyond it every reference is a constant or an exact 0, and between 5 and 10 pixels the
only term of dx is the tiny G*dmu.  On the structural families (``flat``, ``identical``) d/dmu1 and dx are differences of equal terms:
their reference is 0 wherever x == y over the window, so vacuity says nothing there; instead the bound must be small against what
cancels, bound <= k m with m the expression evaluated with absolute values (``E.m``: sums of |terms|, products of magnitudes; a
division by b amplifies by m_b / |b|) and k = 2 n u, n the roundings on the expression's longest path (``E.n``).

**The float32 restatement** (``restate_loss_forward`` / ``_backward``, ``restate_metrics``) follows the kernels tile by tile: staging
with the apron origin, horizontal then vertical pass with taps ascending from 0, the epilogues in source order (``fused=True``: every
product fused into the following add / subtract), the thread / wave / workgroup sums, the owner rule of the metrics' L1 sums.
float32 FMAs are formed as the float64 product (exact) + addend rounded to float64 and then to float32; the double rounding can
differ from a true FMA by an ulp in rare ties, which is why only the pools (no FMA) are compared bit for bit.
"""
import math

import numpy as np

from tests import metrics_ref as MR

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
VACUITY_CAP = 0.01
f32 = np.float32
T_W, T_H, RAD, TAPS, APRON = 32, 64, 5, 11, 10      # csrc/ssim_window.h: SW_T, SW_TH, SW_R, SW_TAPS, SW_A
S_W, S_H = T_W + APRON, T_H + APRON                 # staged columns / rows: 42 x 74
C1_32, C2_32 = f32(0.01) * f32(0.01), f32(0.03) * f32(0.03)     # loss.hip: 0.01f * 0.01f, 0.03f * 0.03f
C1_M, C2_M = f32(0.01 * 0.01), f32(0.03 * 0.03)                 # metrics.hip: (float)(0.01 * 0.01), (float)(0.03 * 0.03)
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


class Denominator(AssertionError):
    """A divisor's bound reaches half the divisor: the quotient's first-order bound does not hold for this input."""


# ---- windows ------------------------------------------------------------------------------------------------------------------
def win_f32():
    """fill_window_f32: float32 exps, serial float32 sum, float32 divide."""
    g = np.array([f32(math.exp(-float((k - RAD) * (k - RAD)) / (2.0 * 1.5 * 1.5))) for k in range(TAPS)], dtype=f32)
    s = f32(0.0)
    for k in range(TAPS):
        s = f32(s + g[k])
    return (g / s).astype(f32)


def win_f64():
    """fill_window_f64: normalised in float64, rounded once."""
    g = np.array([math.exp(-float((k - RAD) * (k - RAD)) / (2.0 * 1.5 * 1.5)) for k in range(TAPS)])
    return (g / g.sum()).astype(f32)


def window_distance():
    """Largest |trainer's tap - exact product| / (u * product) over the 121 taps (the trainer rounds the outer product once)."""
    w = win_f32()
    exact = np.outer(w.astype(np.float64), w.astype(np.float64))
    trainer = np.outer(w, w).astype(f32).astype(np.float64)
    return float((np.abs(trainer - exact) / (U * exact)).max())


def conv64(a, w, pad=True):
    """The separable window in float64 over the last two axes: zero padded (centred) or valid."""
    a = np.asarray(a, np.float64)
    w = np.asarray(w, np.float64)
    if pad:
        p = np.zeros(a.shape[:-2] + (a.shape[-2] + APRON, a.shape[-1] + APRON))
        p[..., RAD:RAD + a.shape[-2], RAD:RAD + a.shape[-1]] = a
        a = p
    H, W = a.shape[-2] - APRON, a.shape[-1] - APRON
    h = sum(w[k] * a[..., :, k:k + W] for k in range(TAPS))
    return sum(w[k] * h[..., k:k + H, :] for k in range(TAPS))


# ---- running error ------------------------------------------------------------------------------------------------------------
class E:
    """value, error bound, magnitude (the expression with absolute values), roundings on the longest path."""

    def __init__(self, v, e=0.0, m=None, n=0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) + e
        self.m = np.abs(self.v) if m is None else np.zeros_like(self.v) + m
        self.n = n

    def _rounded(self, v, e, m, n):
        return E(v, e + U * (np.abs(v) + e), m, n + 1)

    def __neg__(self):
        return E(-self.v, self.e, self.m, self.n)

    def __add__(self, o):
        return self._rounded(self.v + o.v, self.e + o.e, self.m + o.m, max(self.n, o.n))

    def __sub__(self, o):
        return self + (-o)

    def __mul__(self, o):
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e, self.m * o.m, self.n + o.n)

    def __truediv__(self, o):
        lo = np.abs(o.v) - o.e
        if not bool((lo > 0.5 * np.abs(o.v)).all()):
            raise Denominator("bound / |divisor| reaches %.3g" % float((o.e / np.abs(o.v)).max()))
        q = self.v / o.v
        return self._rounded(q, (self.e + np.abs(q) * o.e) / lo, self.m * o.m / (np.abs(o.v) * lo), self.n + o.n)

    def times(self, c):
        """... by a power of two: exact."""
        return E(self.v * c, self.e * abs(c), self.m * abs(c), self.n)

    @property
    def bound(self):
        return self.e * SLACK


def _windowed(src, w, n, pad):
    """G*v of inputs ``src`` (an E: exact values have e = 0), after n roundings on a term of the window's sum."""
    mag = conv64(np.abs(src.v), w, pad)
    spread = conv64(src.e, w, pad) if np.any(src.e) else np.zeros_like(mag)
    return E(conv64(src.v, w, pad), n * U * (mag + spread) + spread, conv64(src.m, w, pad), n + src.n)


def _const(c, like):
    return E(np.full(like.shape, float(c)))


# ---- the loss: float64 reference ------------------------------------------------------------------------------------------------
def loss_reference(x, y, win=None):
    """x, y: (C, H, W) float32.  -> dict of E: ssim, the three maps ``dmu``, ``de11``, ``de12`` and ``ad`` = |x - y|."""
    w = (win_f32() if win is None else win).astype(np.float64)
    X, Y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x_, y_ = E(X), E(Y)
    m1, m2 = _windowed(x_, w, 22, True), _windowed(y_, w, 22, True)
    e11, e22, e12 = _windowed(x_ * x_, w, 22, True), _windowed(y_ * y_, w, 22, True), _windowed(x_ * y_, w, 22, True)
    C1, C2 = _const(C1_32, X), _const(C2_32, X)
    mu1_sq, mu2_sq, mu12 = m1 * m1, m2 * m2, m1 * m2
    s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    A, B = mu12.times(2) + C1, s12.times(2) + C2
    Cc, D = (mu1_sq + mu2_sq) + C1, (s1 + s2) + C2
    inv = _const(1.0, X) / (Cc * D)
    ssim = (A * B) * inv
    t1 = (m2.times(2) * (B - A)) * inv
    t2 = ((ssim.times(2) * m1) * (D - Cc)) * inv
    d = X - Y
    return {"ssim": ssim, "dmu": t1 - t2, "de11": (-ssim) / D, "de12": A.times(2) * inv, "ad": E(np.abs(d), U * np.abs(d), None, 1),
            "moments": (m1.v, m2.v, e11.v, e22.v, e12.v)}


def n_blocks(C, H, W):
    return C * (-(-H // T_H)) * (-(-W // T_W))


def state_floats(C, H, W):
    return 3 * C * H * W + 2 * n_blocks(C, H, W)


def tile_sums(a):
    """(C, H, W) float64 -> the per-workgroup sums in the partials' order: ((c * gy) + by) * gx + bx."""
    C, H, W = a.shape
    return np.array([a[c, by:by + T_H, bx:bx + T_W].sum() for c in range(C) for by in range(0, H, T_H) for bx in range(0, W, T_W)])


def partial_reference(ref):
    """-> (value [blocks][2], bound [blocks][2]): sum |x - y| and sum ssim_map per workgroup."""
    out = []
    for k in ("ad", "ssim"):
        v, e = tile_sums(ref[k].v), tile_sums(ref[k].e)
        out.append((v, (e + 13 * U * tile_sums(np.abs(ref[k].v) + ref[k].e)) * SLACK))
    return np.stack([out[0][0], out[1][0]], 1), np.stack([out[0][1], out[1][1]], 1)


def out3_from_partials(partial, n, lam):
    """The finish kernel from the kernel's own partials (float32, [blocks][2]) -> (value (3,), bound (3,))."""
    p = np.asarray(partial, np.float64)
    v = p.sum(0) / n
    b = (U * np.abs(v) + 1e-15 * np.abs(p).sum(0) / n) * SLACK
    return np.append(v, 0.0), np.append(b, 0.0)


def out3_combined(l1, ss, lam):
    """out3[2] from the float32 out3[0], out3[1] and the float32 lambda -> (value, bound)."""
    lam = float(f32(lam))
    a, b = (1.0 - lam) * float(l1), lam * (1.0 - float(ss))
    return a + b, 3 * U * (abs(a) + abs(b)) * SLACK


def out3_end_to_end(ref, n, lam):
    pv, pb = partial_reference(ref)
    v = pv.sum(0) / n
    b = pb.sum(0) / n + U * np.abs(v) * SLACK
    lam = float(f32(lam))
    c, cb = out3_combined(v[0], v[1], lam)
    return np.append(v, c), np.append(b, cb + (1.0 - lam) * b[0] + lam * b[1])


def effective_g(g, lam):
    """(gl, gs) as E scalars from the device scalars g = (g_l1, g_ssim, g_loss), each None or a float32, as the kernel forms them."""
    gl1, gss, glo = (E(0.0) if v is None else E(float(f32(v))) for v in g)
    lam = E(float(f32(lam)))
    return gl1 + (E(1.0) - lam) * glo, gss - lam * glo


def split_route(lam, g_loss):
    """The (g_l1, g_ssim, NULL) with the effective coefficients of (NULL, NULL, g_loss): (1 - lambda) g_loss and -lambda g_loss in float32."""
    lam, gt = f32(lam), f32(g_loss)
    return (f32(1.0) - lam) * gt, -(lam * gt), None


def routes_agree(x, y, state, lam, g_loss, dx_loss, dx_split):
    """|dx by the g_loss route - dx by the g_l1 / g_ssim route| within the two stage bounds (+ the distance of the two references)."""
    C, H, W = x.shape
    maps = [E(np.asarray(state[:3 * x.size], f32).reshape(3, C, H, W)[k]) for k in range(3)]
    a, b = dx_reference(x, y, maps, lam, (None, None, g_loss)), dx_reference(x, y, maps, lam, split_route(lam, g_loss))
    return bool((np.abs(np.asarray(dx_loss, np.float64) - dx_split) <= a.bound + b.bound + np.abs(a.v - b.v)).all())


def dx_reference(x, y, maps, lam, g, win=None):
    """dL/dimage (E) from the three ``maps``, each an E of (C, H, W): exact (the maps the kernel itself wrote) or with their bounds."""
    w = (win_f32() if win is None else win).astype(np.float64)
    X, Y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    cv = [_windowed(maps[k], w, 22, True) for k in range(3)]
    n = X.size
    inv_n = E(np.full(X.shape, 1.0 / n), U / n, None, 1)
    gl, gs = effective_g(g, lam)
    gl, gs = (E(np.full(X.shape, float(t.v)), float(t.e), float(t.m), t.n) for t in (gl, gs))
    t = (cv[0] + E(2.0 * X) * cv[1]) + E(Y) * cv[2]
    return ((gl * E(np.sign(X - Y))) * inv_n) + ((gs * inv_n) * t)


# ---- the float32 restatement ------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _stage(img, ty0, tx0, org, fault=None):
    """sw_stage of one plane: 74 x 42 pixels from (ty0 + org, tx0 + org); outside the image: 0."""
    H, W = img.shape
    yy, xx = ty0 + org + np.arange(S_H), tx0 + org + np.arange(S_W)
    v = img[np.clip(yy, 0, H - 1)][:, np.clip(xx, 0, W - 1)].astype(f32)
    if fault != "clamp_to_edge":
        ok = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
        v = np.where(ok, v, f32(0.0))
    if fault == "apron_col_41":
        v[:, S_W - 1] = 0.0
    if fault == "apron_row_73":
        v[S_H - 1, :] = 0.0
    return v


def _taps(v, win, axis, drop=None):
    """One pass over `axis` of (..., rows, columns): accumulators from 0, taps ascending."""
    n = v.shape[axis] - APRON
    acc = None
    for k in range(TAPS):
        sl = v[..., k:k + n] if axis == -1 else v[..., k:k + n, :]
        if acc is None:
            acc = np.zeros(sl.shape, f32)
        if k != drop:
            acc = fma32(win[k], sl, acc)
    return acc


def _window_tile(planes, win, fault=None):
    """(P, 74, 42) staged -> (P, 64, 32): horizontal, then vertical."""
    h = _taps(planes, win, -1, 0 if fault == "h_tap_0" else None)
    return _taps(h, win, -2, 10 if fault == "v_tap_10" else None)


def _wg_sum32(v):
    """(64, 32) float32 -> the workgroup's sum as the kernel forms it: thread = (column, 4 consecutive rows) adds its four serially
    from 0, the wave (2 x 32 threads) in six pairwise steps, the eight waves as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7))."""
    t = v.reshape(T_H // 4, 4, T_W)
    s = np.zeros((T_H // 4, T_W), f32)
    for o in range(4):
        s = s + t[:, o, :]
    lanes = s.reshape(8, 64)
    while lanes.shape[1] > 1:
        lanes = lanes[:, 0::2] + lanes[:, 1::2]
    r = lanes[:, 0]
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))


def _loss_fwd_epilogue(m1, m2, e11, e22, e12, fault=None, fused=False):
    C1, C2 = (C2_32, C1_32) if fault == "c1_c2_exchanged" else (C1_32, C2_32)
    two, one = f32(2.0), f32(1.0)
    mu1_sq, mu2_sq, mu12 = m1 * m1, m2 * m2, m1 * m2
    if fused:
        s1, s2, s12 = fma32(-m1, m1, e11), fma32(-m2, m2, e22), fma32(-m1, m2, e12)
        Cc = fma32(m1, m1, mu2_sq) + C1
    else:
        s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
        Cc = mu1_sq + mu2_sq + C1
    A, B, D = two * mu12 + C1, two * s12 + C2, s1 + s2 + C2
    inv = one / (Cc * D)
    ssim = A * B * inv
    t1 = two * m2 * (B - A) * inv
    t2 = (two * m1 if fault == "dmu_without_ssim" else ssim * two * m1) * (D - Cc)
    dmu = fma32(-t2, inv, t1) if fused else t1 - t2 * inv
    return ssim, dmu, -ssim / D, two * A * inv


def restate_loss_forward(x, y, lam, fault=None, fused=False, win=None):
    """-> (state: float32 [state_floats], NaN where nothing was written; out3: float32 (3,))."""
    win = win_f32() if win is None else win
    C, H, W = x.shape
    org = -4 if fault == "origin_-4" else -RAD
    plane = (H * W if fault == "plane_stride_hw" else C * H * W)
    state = np.full(state_floats(C, H, W), np.nan, f32)
    part = state[3 * C * H * W:].reshape(-1, 2)
    gy, gx = -(-H // T_H), -(-W // T_W)
    with np.errstate(all="ignore"):
        for c in range(C):
            for by in range(gy):
                for bx in range(gx):
                    ty0, tx0 = by * T_H, bx * T_W
                    sx, sy = _stage(x[c], ty0, tx0, org, fault), _stage(y[c], ty0, tx0, org, fault)
                    planes = np.stack([sx, sy, sx * sx, sy * sy, sx * sx if fault == "e12_from_xx" else sx * sy])
                    mo = _window_tile(planes, win, fault)
                    ssim, a, b, cc = _loss_fwd_epilogue(*mo, fault=fault, fused=fused)
                    hh, ww = min(T_H, H - ty0), min(T_W, W - tx0)
                    for k, m in enumerate((a, b, cc)):
                        idx = (k * plane + (c * H + ty0 + np.arange(hh)) * W + tx0)[:, None] + np.arange(ww)[None, :]
                        state[idx] = m[:hh, :ww]
                    inside = np.zeros((T_H, T_W), bool)
                    inside[:hh, :ww] = True
                    ad = np.abs(sx[RAD:RAD + T_H, RAD:RAD + T_W] - sy[RAD:RAD + T_H, RAD:RAD + T_W])
                    blk = (c * gy + by) * gx + bx
                    if not (fault == "last_partial_unwritten" and blk == part.shape[0] - 1):
                        part[blk] = (_wg_sum32(np.where(inside, ad, f32(0.0))), _wg_sum32(np.where(inside, ssim, f32(0.0))))
        p = part.astype(np.float64)
        tot = p.sum(0) + (p[0] if fault == "partial_twice" else 0.0)
        n = C * H * W
        l1, ss = f32(tot[0] * (1.0 / n)), f32(tot[1] * (1.0 / n))
        lam = f32(lam)
        out3 = np.array([l1, ss, (f32(1.0) - lam) * l1 + lam * (f32(1.0) - ss)], f32)
    return state, out3


def restate_loss_backward(x, y, state, lam, g, fault=None, fused=False, win=None):
    """-> dx (C, H, W) float32 from the maps in ``state``; g = (g_l1, g_ssim, g_loss), each None (NULL) or a float32."""
    win = win_f32() if win is None else win
    C, H, W = x.shape
    maps = np.asarray(state[:3 * C * H * W], f32).reshape(3, C, H, W)
    dx = np.zeros((C, H, W), f32)
    lam, one, two = f32(lam), f32(1.0), f32(2.0)
    gt = f32(0.0) if g[2] is None else f32(g[2])
    gl = (f32(0.0) if g[0] is None else f32(g[0])) + (one - lam) * gt
    gs = (f32(0.0) if g[1] is None else f32(g[1])) - lam * gt
    inv_n = one / f32(H * W if fault == "inv_n_hw" else C * H * W)
    with np.errstate(all="ignore"):
        for c in range(C):
            for ty0 in range(0, H, T_H):
                for tx0 in range(0, W, T_W):
                    cv = _window_tile(np.stack([_stage(maps[k, c], ty0, tx0, -RAD) for k in range(3)]), win)
                    hh, ww = min(T_H, H - ty0), min(T_W, W - tx0)
                    cv = cv[:, :hh, :ww]
                    xs, ys = x[c, ty0:ty0 + hh, tx0:tx0 + ww], y[c, ty0:ty0 + hh, tx0:tx0 + ww]
                    if fault == "xy_exchanged":
                        xs, ys = ys, xs
                    d = xs - ys
                    sgn = np.sign(d).astype(f32)
                    if fault == "sign_0_plus":
                        sgn = np.where(d == 0, one, sgn)
                    k2 = one if fault == "factor_2_missing" else two
                    if fused:
                        t = fma32(ys, cv[2], fma32(k2 * xs, cv[1], cv[0]))
                        r = fma32(gs * inv_n, t, gl * sgn * inv_n)
                    else:
                        r = gl * sgn * inv_n + gs * inv_n * (cv[0] + k2 * xs * cv[1] + ys * cv[2])
                    dx[c, ty0:ty0 + hh, tx0:tx0 + ww] = r
    return dx


# ---- comparing ---------------------------------------------------------------------------------------------------------------
def compare(got, ref, bound, region=None):
    """-> {n, bad, worst (err / bound), vac, first}: every element |got - ref| <= bound; a NaN is outside."""
    got, ref, bound = (np.asarray(a, np.float64).ravel() for a in (got, ref, np.broadcast_to(bound, np.shape(ref))))
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    bad = ~(err <= bound)
    nz = ref != 0
    if region is not None:
        nz &= np.asarray(region).ravel()
    vac = float((bound[nz] >= np.abs(ref[nz])).mean()) if nz.any() else 0.0
    return {"n": int(ref.size), "bad": int(bad.sum()), "worst": float(ratio.max(initial=0.0)), "vac": vac,
            "first": int(np.argmax(bad)) if bad.any() else -1}


def structural(e, what):
    """bound <= k * magnitude with k = 2 n u -> the worst bound / (k magnitude) (asserted <= 1)."""
    k = 2.0 * e.n * U
    with np.errstate(all="ignore"):
        r = np.where(e.bound == 0, 0.0, e.bound / (k * e.m))
    worst = float(np.max(r, initial=0.0))
    assert worst <= 1.0, "%s: bound / (k magnitude) = %.3g with k = 2 * %d u" % (what, worst, e.n)
    return worst


# ---- input families and the grid of the loss -----------------------------------------------------------------------------------
SCORED = ("noisy", "uniform", "negative", "losstest", "overshoot", "dark")
STRUCTURAL = ("flat", "identical")
FAMILIES = SCORED + STRUCTURAL
LAMBDAS = (0.0, 0.2, 1.0)
G_OPTIONS = tuple((a, b, c) for a in (None, 0.7) for b in (None, -0.3) for c in (None, 1.3))  # (0: all NULL) ... (7: all given)


def dark_mask(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy + 0.5 - H / 2) ** 2 / (H / 3) ** 2 + (xx + 0.5 - W / 2) ** 2 / (W / 3) ** 2) < 1.0


def _dilate(mask, r):
    H, W = mask.shape
    p = np.zeros((H + 2 * r, W + 2 * r), bool)
    p[r:r + H, r:r + W] = mask
    out = np.zeros_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def make_images(shape, family):
    """One seeded float32 (C, H, W) pair: the rendered image x and the ground truth y."""
    C, H, W = shape
    if family in MR.PAIRS:
        x, y = MR.make_pair(shape, family)
        return x[0], y[0]
    if family == "losstest":  # the draw of tests/test_gpu_loss.py::test_against_oracle_ragged_and_full_size
        import torch
        g = torch.Generator().manual_seed(C * 1000 + H)
        gt = torch.rand(C, H, W, generator=g)
        img = (gt + 0.1 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
        return img.numpy(), gt.numpy()
    x, y = MR.make_pair(shape, "noisy")
    x, y = x[0], y[0]
    if family == "overshoot":
        return (x * f32(1.6) - f32(0.3)).astype(f32), (y * f32(1.6) - f32(0.3)).astype(f32)
    if family == "dark":
        m = dark_mask(H, W).astype(f32)
        return (x * m).astype(f32), (y * m).astype(f32)
    if family == "identical":
        return x, x.copy()
    if family == "flat":
        rng = np.random.default_rng([MR.SEED, C, H, W, 7])
        y = rng.random((C, H // 16 + 1, W // 16 + 1)).astype(f32).repeat(16, 1).repeat(16, 2)[:, :H, :W].copy()
        x = y.copy()
        r = W - W // 2
        x[:, :, W // 2:] = np.clip(x[:, :, W // 2:] + f32(0.02) * rng.standard_normal((C, H, r)).astype(f32), 0, 1)
        return x.astype(f32), y
    raise KeyError(family)


def region(shape, family):
    """Where vacuity is counted: everywhere, but for ``dark`` the object plus its 5-pixel rim."""
    C, H, W = shape
    if family != "dark":
        return np.ones(shape, bool)
    return np.broadcast_to(_dilate(dark_mask(H, W), RAD), shape).copy()


WS = (1, 5, 6, 11, 31, 32, 33, 37, 38, 64, 65)
HS = (1, 5, 6, 11, 63, 64, 65, 69, 70, 128, 129)
CS = (1, 3, 4)


def shapes():
    out = []
    for W in WS:
        for H in (1, 11, 65):
            out.append((H, W))
    for H in HS:
        for W in (1, 11, 33):
            if (H, W) not in out:
                out.append((H, W))
    out = [(CS[i % 3], H, W) for i, (H, W) in enumerate(out)]
    return out + [(2, 130, 70), (3, 65, 33), (4, 16, 16)]


def grid():
    """Every shape with two families (so every family runs on well over three shapes), lambda and the backward's option dealt
    round-robin (options 1..7: at least one upstream gradient given).  ``negative`` is dealt g_l1 = 0.7 and g_loss = 1.3 at lambda
    0.2 (gl = 1.74, gs = -0.26) throughout: with anticorrelated images the three convolved maps cancel to a few percent of their terms, and the end-to-end
    bound of an ssim-only gradient reached |reference| on up to 6 % of the pixels, of gl = 0.7, gs = -0.3 on up to 1.9 % (the cap is
    1 %: the input changes, not the cap); the ssim-only routes on that family are held by the stage check of the option tests."""
    out = []
    for i, shape in enumerate(shapes()):
        for j in range(2):
            k = 2 * i + j
            fam = FAMILIES[(i + 3 * j + i // len(FAMILIES)) % len(FAMILIES)]
            lam, opt = LAMBDAS[k % 3], 1 + k % 7
            if fam == "negative":
                lam, opt = 0.2, 5
            out.append({"name": "%dx%dx%d %s" % (shape + (fam,)), "shape": shape, "family": fam, "lam": lam, "g": G_OPTIONS[opt]})
    return out


LOSS_ARRAYS = ("dmu", "de11", "de12", "partial_l1", "partial_ssim", "out3", "out3_e2e", "dx_stage", "dx_e2e")


def check_loss(case, x, y, state, out3, dx, g=None, ref=None, win=None):
    """Every array of one forward + backward against its reference.  ``state``: the float32 buffer of exactly state_floats;
    -> {array: compare(...)} plus the entries ``nan_free`` and ``structural`` (worst bound / (k magnitude), structural families)."""
    C, H, W = x.shape
    n, lam, fam = C * H * W, case["lam"], case["family"]
    g = case["g"] if g is None else g
    ref = loss_reference(x, y, win) if ref is None else ref
    reg = region(x.shape, fam)
    maps = np.asarray(state[:3 * n], f32).reshape(3, C, H, W)
    part = np.asarray(state[3 * n:], f32).reshape(-1, 2)
    res = {}
    for k, name in enumerate(("dmu", "de11", "de12")):
        res[name] = compare(maps[k], ref[name].v, ref[name].bound, reg)
    pv, pb = partial_reference(ref)
    res["partial_l1"] = compare(part[:, 0], pv[:, 0], pb[:, 0])
    res["partial_ssim"] = compare(part[:, 1], pv[:, 1], pb[:, 1])
    ov, ob = out3_from_partials(part, n, lam)
    ov[2], ob[2] = out3_combined(out3[0], out3[1], lam)
    res["out3"] = compare(out3, ov, ob)
    ev, eb = out3_end_to_end(ref, n, lam)
    res["out3_e2e"] = compare(out3, ev, eb)
    stage = dx_reference(x, y, [E(maps[k]) for k in range(3)], lam, g, win)
    res["dx_stage"] = compare(dx, stage.v, stage.bound, reg)
    e2e = dx_reference(x, y, [ref[k] for k in ("dmu", "de11", "de12")], lam, g, win)
    res["dx_e2e"] = compare(dx, e2e.v, e2e.bound, reg)
    res["nan_free"] = not bool(np.isnan(np.asarray(state)).any())
    if fam == "identical":   # the reference is 0: |dx| within its bound
        res["dx_zero"] = compare(dx, np.zeros(x.shape), e2e.bound + np.abs(e2e.v))
        res["dx_zero"]["vac"] = 0.0
    if fam in STRUCTURAL:
        res["structural"] = max(structural(ref["dmu"], "dmu"), structural(stage, "dx_stage"), structural(e2e, "dx_e2e"))
        for k in ("dmu", "dx_stage", "dx_e2e"):
            res[k]["vac"] = 0.0   # (not counted: the reference is 0 wherever x == y over the window)
    return res


def bad_arrays(res):
    out = sorted(k for k, v in res.items() if isinstance(v, dict) and v["bad"])
    if res.get("nan_free") is False:
        out.append("nan_free")
    return out


def vacuous_arrays(res):
    return {k: v["vac"] for k, v in res.items() if isinstance(v, dict) and v["vac"] > VACUITY_CAP}


def restate_case(case, fault=None, fused=False, win=None, g=None):
    x, y = make_images(case["shape"], case["family"])
    fwd = fault if fault not in BACKWARD_FAULTS else None
    state, out3 = restate_loss_forward(x, y, case["lam"], fwd, fused, win)
    dx = restate_loss_backward(x, y, state, case["lam"], case["g"] if g is None else g, fault if fault in BACKWARD_FAULTS else None, fused,
                               win)
    return x, y, state, out3, dx


BACKWARD_FAULTS = ("factor_2_missing", "xy_exchanged", "sign_0_plus", "inv_n_hw")
_FWD_ALL = {"dmu", "de11", "de12", "partial_ssim", "out3_e2e", "dx_e2e"}
# fault -> (shape, family, lambda, g option, the arrays it spoils)
LOSS_FAULTS = {
    "h_tap_0": ((1, 65, 33), "noisy", 0.2, 7, _FWD_ALL),
    "v_tap_10": ((1, 65, 33), "noisy", 0.2, 7, _FWD_ALL),
    "origin_-4": ((1, 65, 33), "noisy", 0.2, 7, _FWD_ALL | {"partial_l1"}),
    "clamp_to_edge": ((3, 11, 38), "uniform", 0.2, 7, _FWD_ALL),
    "apron_col_41": ((1, 11, 38), "uniform", 0.2, 7, _FWD_ALL),
    "apron_row_73": ((1, 70, 11), "uniform", 0.2, 7, _FWD_ALL),
    "c1_c2_exchanged": ((1, 65, 33), "noisy", 0.2, 7, _FWD_ALL),
    "e12_from_xx": ((1, 65, 33), "noisy", 0.2, 7, _FWD_ALL - {"de12"}),   # (d/dE[xy] = 2 A / (Cc D) does not read E[xy])
    "dmu_without_ssim": ((1, 65, 33), "noisy", 0.2, 7, {"dmu", "dx_e2e"}),
    "plane_stride_hw": ((3, 65, 33), "noisy", 0.2, 7, {"de11", "de12", "dx_stage", "dx_e2e", "nan_free"}),
    "factor_2_missing": ((1, 65, 33), "noisy", 0.2, 7, {"dx_stage", "dx_e2e"}),
    "xy_exchanged": ((1, 65, 33), "noisy", 0.2, 7, {"dx_stage", "dx_e2e"}),
    "sign_0_plus": ((1, 65, 33), "flat", 0.2, 7, {"dx_stage", "dx_e2e"}),
    "inv_n_hw": ((3, 65, 33), "noisy", 0.2, 7, {"dx_stage", "dx_e2e"}),
    "last_partial_unwritten": ((2, 130, 70), "noisy", 0.2, 7, {"partial_l1", "partial_ssim", "out3", "out3_e2e", "nan_free"}),
    "partial_twice": ((2, 130, 70), "noisy", 0.2, 7, {"out3", "out3_e2e"}),
}


def fault_case(fault):
    shape, fam, lam, opt, spoils = LOSS_FAULTS[fault]
    return {"name": fault, "shape": shape, "family": fam, "lam": lam, "g": G_OPTIONS[opt]}, spoils


def old_bars_loss(x, y, out3, dx, g):
    """Would tests/test_gpu_loss.py's bars reject this result?  1e-4 of the gradient's largest entry, 5e-6 on the ssim mean, 1e-6 on
    l1, against oracle/loss_ref.py."""
    from oracle import loss_ref as O
    gl, gs = effective_g(g, 0.2)
    want = O.grad(x, y, float(gl.v), float(gs.v))
    return not bool(np.abs(dx - want).max() <= 1e-4 * np.abs(want).max() and abs(float(out3[1]) - O.ssim(x, y)) < 5e-6
                    and abs(float(out3[0]) - O.l1(x, y)) < 1e-6)


# ---- the metrics -------------------------------------------------------------------------------------------------------------
def plan(B, C, H, W):
    """metrics_plan (csrc/metrics.hip) restated: the pyramid's sizes and where everything lives in the workspace — the float64
    partials first, level by level ([plane][workgroup][4]; offsets ``part`` in doubles), then the pyramid images of levels 1..5
    (offsets ``img`` in floats; x's planes, then y's)."""
    m = min(H, W)
    planes = B * C
    q, r = divmod(m, 256)
    f = max(1, q + (1 if (r > 128 or (r == 128 and q & 1)) else 0))
    ms = m > 160
    h, w = [H], [W]
    for l in range(1, 5):
        h.append((h[-1] + 1) // 2 if ms else 0)
        w.append((w[-1] + 1) // 2 if ms else 0)
    h.append(H // f)
    w.append(W // f)
    tx, ty, part, img = [0] * 6, [0] * 6, [0] * 6, [0] * 6
    d = 0
    for l in range(6):
        runs = h[l] >= TAPS and w[l] >= TAPS
        tx[l] = -(-(w[l] - APRON) // T_W) if runs else 0
        ty[l] = -(-(h[l] - APRON) // T_H) if runs else 0
        if l == 5 and f == 1:
            part[5] = part[0]
            break
        part[l] = d
        d += planes * tx[l] * ty[l] * 4
    fl = 2 * d
    for l in range(1, 6):
        if l == 5 and f == 1:
            break
        img[l] = fl
        fl += 2 * planes * h[l] * w[l]
    return {"f": f, "ms": ms, "h": h, "w": w, "tx": tx, "ty": ty, "part": part, "img": img, "doubles": d, "total_floats": fl,
            "planes": planes}


def restate_pool(x, k, ph=0, pw=0, clamp=False, fault=None):
    """metrics_pool_kernel of (planes, h, w) float32: serial adds over di, dj, one division.  Bit for bit."""
    P, h, w = x.shape
    oh, ow = (h + ph) // k, (w + pw) // k
    p = np.zeros((P, h + ph, w + pw), f32)
    if fault == "pool_pad_behind":
        p[:, :h, :w] = x
    else:
        p[:, ph:, pw:] = x
    if clamp:
        p = np.minimum(np.maximum(p, f32(0.0)), f32(1.0))
    acc = np.zeros((P, oh, ow), f32)
    for di in range(k):
        for dj in range(k):
            acc = acc + p[:, di:oh * k:k, dj:ow * k:k]
    return acc / f32(k * k)


def pool64(x, k, ph=0, pw=0):
    """-> (value, bound): the same pool of float32 values in float64; k^2 roundings."""
    P, h, w = x.shape
    oh, ow = (h + ph) // k, (w + pw) // k
    p = np.zeros((P, h + ph, w + pw))
    p[:, ph:, pw:] = x
    v = sum(p[:, di:oh * k:k, dj:ow * k:k] for di in range(k) for dj in range(k)) / (k * k)
    a = sum(np.abs(p[:, di:oh * k:k, dj:ow * k:k]) for di in range(k) for dj in range(k)) / (k * k)
    return v, k * k * U * a * SLACK


def restate_level(x, y, clamp=False, first=True, fault=None, fused=False):
    """metrics_level_kernel of one plane pair (h, w) float32 -> float64 [workgroups][4]."""
    win = win_f64()
    h, w = x.shape
    gx, gy = -(-(w - APRON) // T_W), -(-(h - APRON) // T_H)
    out = np.zeros((gy * gx, 4))
    half, two = f32(0.5), f32(2.0)
    with np.errstate(all="ignore"):
        for by in range(gy):
            for bx in range(gx):
                ty0, tx0 = by * T_H, bx * T_W
                vx, vy = _stage(x, ty0, tx0, 0), _stage(y, ty0, tx0, 0)
                if clamp:
                    vx, vy = (np.minimum(np.maximum(v, f32(0.0)), f32(1.0)) for v in (vx, vy))
                sx, sy = vx - half, vy - half
                r, q = np.arange(S_H)[:, None], np.arange(S_W)[None, :]
                owned = (ty0 + r < h) & (tx0 + q < w)
                if fault != "apron_owned_twice":
                    owned = owned & ((r < T_H) | (by == gy - 1)) & ((q < T_W) | (bx == gx - 1))
                d = vx - vy
                d2 = d * d
                ad, sq = (np.abs(d).astype(np.float64)[owned].sum(), d2.astype(np.float64)[owned].sum()) if first else (0.0, 0.0)
                m1, m2, e11, e22, e12 = _window_tile(np.stack([sx, sy, sx * sx, sy * sy, sx * sy]), win)
                if fused:
                    s1, s2, s12 = fma32(-m1, m1, e11), fma32(-m2, m2, e22), fma32(-m1, m2, e12)
                else:
                    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
                mu1, mu2 = (m1, m2) if fault == "mu_without_shift" else (m1 + half, m2 + half)
                mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
                cs = (two * s12 + C2_M) / (s1 + s2 + C2_M)
                den = (fma32(mu1, mu1, mu2_sq) if fused else mu1_sq + mu2_sq) + C1_M
                ss = (two * mu12 + C1_M) / den * cs
                valid = ((ty0 + np.arange(T_H)) < h - APRON)[:, None] & ((tx0 + np.arange(T_W)) < w - APRON)[None, :]
                out[by * gx + bx] = (ss.astype(np.float64)[valid].sum(), cs.astype(np.float64)[valid].sum(), ad, sq)
    return out


def level_reference(x, y):
    """The shifted form in float64 of one plane pair (float32, already clamped) -> (ssim_map E, cs_map E) over the valid outputs."""
    w = win_f64().astype(np.float64)
    X, Y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    sx, sy = (E(v - 0.5, np.where((v >= 0.25) & (v <= 2.0), 0.0, U * np.abs(v - 0.5)), None, 1) for v in (X, Y))
    m1, m2 = _windowed(sx, w, 22, False), _windowed(sy, w, 22, False)
    e11, e22, e12 = _windowed(sx * sx, w, 22, False), _windowed(sy * sy, w, 22, False), _windowed(sx * sy, w, 22, False)
    like = m1.v
    C1, C2, half = _const(C1_M, like), _const(C2_M, like), _const(0.5, like)
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    mu1, mu2 = m1 + half, m2 + half
    cs = (s12.times(2) + C2) / ((s1 + s2) + C2)
    ss = (((mu1 * mu2).times(2) + C1) / ((mu1 * mu1 + mu2 * mu2) + C1)) * cs
    return ss, cs


def level_partial_reference(x, y):
    """-> (value, bound) [workgroups][2]: the tile sums of ssim_map and cs_map."""
    ss, cs = level_reference(x, y)
    out = []
    for e in (ss, cs):
        v, b = tile_sums(e.v[None]), tile_sums(e.bound[None]) + 1e-13 * tile_sums(np.abs(e.v[None]))
        out.append((v, b))
    return np.stack([out[0][0], out[1][0]], 1), np.stack([out[0][1], out[1][1]], 1)


def pyramid(x, y, clamp, want_ms, fault=None):
    """The level images of (planes, H, W) float32 inputs as the launches make them: {level: (x planes, y planes, clamp on load)}."""
    P, H, W = x.shape
    p = plan(1, P, H, W)
    lv = {0: (x, y, clamp)}
    if want_ms:
        for l in range(1, 5):
            px, py, cl = lv[l - 1]
            ph, pw = p["h"][l - 1] % 2, p["w"][l - 1] % 2
            lv[l] = (restate_pool(px, 2, ph, pw, cl and l == 1, fault), restate_pool(py, 2, ph, pw, cl and l == 1, fault), False)
    if p["f"] > 1:
        lv[5] = (restate_pool(x, p["f"], 0, 0, clamp, fault), restate_pool(y, p["f"], 0, 0, clamp, fault), False)
    return p, lv


def finish_from_partials(p, partial, B, C, want_ms):
    """metrics_finalise_kernel in float64 from the partials (float64 [doubles]) -> (out (B, 4), levels (B, 6, C, 2)) before the cast."""
    out, levels = np.full((B, 4), np.nan), np.full((B, 6, C, 2), np.nan)
    active = [True] + [bool(want_ms)] * 4 + [True]
    with np.errstate(all="ignore"):
        for b in range(B):
            ad = sq = ssim_tot = ms_tot = 0.0
            for c in range(C):
                prod = 1.0
                for l in range(6):
                    if not active[l]:
                        continue
                    src = 0 if (l == 5 and p["f"] == 1) else l
                    nwg = p["tx"][src] * p["ty"][src]
                    o = p["part"][l] + (b * C + c) * nwg * 4
                    v = np.asarray(partial[o:o + nwg * 4], np.float64).reshape(nwg, 4).sum(0)
                    cnt = float(p["h"][src] - APRON) * float(p["w"][src] - APRON)
                    mean_ss, mean_cs = v[0] / cnt, v[1] / cnt
                    levels[b, l, c] = (mean_ss, mean_cs)
                    if l == 0:
                        ad, sq = ad + v[2], sq + v[3]
                    if l < 4:
                        prod *= max(mean_cs, 0.0) ** MS_WEIGHTS[l]
                    elif l == 4:
                        prod *= max(mean_ss, 0.0) ** MS_WEIGHTS[4]
                    else:
                        ssim_tot += mean_ss
                ms_tot += prod
            n = float(p["h"][0]) * p["w"][0] * C
            mse = sq / n
            out[b] = (ad / n, np.inf if mse == 0 else 20.0 * math.log10(1.0 / math.sqrt(mse)), ssim_tot / C, ms_tot / C if want_ms else np.nan)
    return out, levels


def restate_metrics(x, y, clamp, want_ms, fault=None, fused=False):
    """riggs_image_metrics of (B, C, H, W) float32 -> {"partial": float64 [doubles], "img": {level: (2, planes, h, w)}, "out", "levels"}."""
    B, C, H, W = x.shape
    p = plan(B, C, H, W)
    _, lv = pyramid(x.reshape(B * C, H, W), y.reshape(B * C, H, W), clamp, want_ms, fault)
    partial = np.zeros(p["doubles"])
    for l, (lx, ly, cl) in lv.items():
        nwg = p["tx"][l] * p["ty"][l]
        for pl in range(B * C):
            o = p["part"][l] + pl * nwg * 4
            partial[o:o + nwg * 4] = restate_level(lx[pl], ly[pl], cl, l == 0, fault, fused).ravel()
    out, levels = finish_from_partials(p, partial, B, C, want_ms)
    return {"partial": partial, "img": {l: np.stack([v[0], v[1]]) for l, v in lv.items() if l > 0}, "out": out.astype(f32),
            "levels": levels.astype(f32)}


def split_workspace(ws, B, C, H, W, want_ms):
    """The caller's workspace (float32 array of total_floats) -> the restatement's {"partial", "img"} views."""
    p = plan(B, C, H, W)
    ws = np.ascontiguousarray(ws, f32)
    img = {}
    for l in ([1, 2, 3, 4] if want_ms else []) + ([5] if p["f"] > 1 else []):
        n = p["planes"] * p["h"][l] * p["w"][l]
        img[l] = ws[p["img"][l]:p["img"][l] + 2 * n].reshape(2, p["planes"], p["h"][l], p["w"][l])
    return {"partial": ws[:2 * p["doubles"]].view(np.float64), "img": img}


METRICS_ARRAYS = ("pool_bits", "pool", "part_ssim", "part_cs", "part_ad", "part_sq", "levels", "out")


def _cast_check(got, want):
    """One cast of a float64 value (2 u allowed); NaN and inf must agree exactly."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    fin = np.isfinite(want)
    same = np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    r = compare(got[fin], want[fin], 2 * U * np.abs(want[fin]))
    if not same:
        r["bad"] += 1
        r["worst"] = np.inf
    return r


def check_metrics(x, y, clamp, want_ms, got):
    """``got``: {"partial", "img", "out", "levels"} of the kernel (or the restatement).  x, y (B, C, H, W) float32."""
    B, C, H, W = x.shape
    p, lv = pyramid(x.reshape(B * C, H, W), y.reshape(B * C, H, W), clamp, want_ms)
    res = {}
    bits = {"n": 0, "bad": 0, "worst": 0.0, "vac": 0.0, "first": -1}
    pool = dict(bits)
    for l in sorted(got["img"]):
        for s in range(2):
            # bit for bit against the float32 restatement FROM THE KERNEL'S OWN source level, and 4 u / k^2 u against float64
            src = 0 if l in (1, 5) else l - 1
            k = p["f"] if l == 5 else 2
            ph, pw = (0, 0) if l == 5 else (p["h"][src] % 2, p["w"][src] % 2)
            base = (x, y)[s].reshape(B * C, H, W) if src == 0 else np.asarray(got["img"][src][s], f32)
            cl = bool(clamp) and src == 0
            want = restate_pool(base, k, ph, pw, cl)
            g = np.asarray(got["img"][l][s], f32)
            bits["n"] += g.size
            bits["bad"] += int((g.view(np.uint32) != want.view(np.uint32)).sum())
            bits["worst"] = float(bits["bad"] > 0)
            b64 = np.minimum(np.maximum(base, f32(0.0)), f32(1.0)) if cl else base
            r = compare(g, *pool64(b64, k, ph, pw))
            pool = {"n": pool["n"] + r["n"], "bad": pool["bad"] + r["bad"], "worst": max(pool["worst"], r["worst"]),
                    "vac": max(pool["vac"], r["vac"]), "first": r["first"]}
    res["pool_bits"], res["pool"] = bits, pool
    acc = {k: [] for k in ("part_ssim", "part_cs", "part_ad", "part_sq")}
    for l, (lx, ly, cl) in lv.items():
        nwg = p["tx"][l] * p["ty"][l]
        for pl in range(B * C):
            o = p["part"][l] + pl * nwg * 4
            gp = np.asarray(got["partial"][o:o + nwg * 4], np.float64).reshape(nwg, 4)
            # the level kernel's input is what the kernel's own pool wrote
            ix, iy = (lx[pl], ly[pl]) if l == 0 else (np.asarray(got["img"][l][0][pl], f32), np.asarray(got["img"][l][1][pl], f32))
            if cl:
                ix, iy = (np.minimum(np.maximum(v, f32(0.0)), f32(1.0)) for v in (ix, iy))
            v, b = level_partial_reference(ix, iy)
            acc["part_ssim"].append(compare(gp[:, 0], v[:, 0], b[:, 0]))
            acc["part_cs"].append(compare(gp[:, 1], v[:, 1], b[:, 1]))
            r = restate_level(ix, iy, False, l == 0)
            for k, col in (("part_ad", 2), ("part_sq", 3)):
                acc[k].append(compare(gp[:, col], r[:, col], 1e-12 * np.abs(r[:, col])))
    for k, rs in acc.items():
        res[k] = {"n": sum(r["n"] for r in rs), "bad": sum(r["bad"] for r in rs), "worst": max(r["worst"] for r in rs),
                  "vac": max(r["vac"] for r in rs), "first": -1}
    out, levels = finish_from_partials(p, got["partial"], B, C, want_ms)
    res["levels"], res["out"] = _cast_check(got["levels"], levels), _cast_check(got["out"], out)
    return res


# (name, (C, H, W), family, want_ms): the shapes of the partials — one output; on, and one over, a tile of outputs; two planes;
# five levels down to a single output; a ragged two-by-three grid of workgroups; the pool by f = 2
METRICS_CASES = (
    ("1x11x11 noisy", (1, 11, 11), "noisy", False),
    ("1x74x42 uniform", (1, 74, 42), "uniform", False),
    ("1x75x43 noisy", (1, 75, 43), "noisy", False),
    ("2x43x12 negative", (2, 43, 12), "negative", False),
    ("3x161x161 noisy", (3, 161, 161), "noisy", True),
    ("1x176x163 uniform", (1, 176, 163), "uniform", True),
    ("1x385x385 noisy", (1, 385, 385), "noisy", True),
)
# fault -> (case name, the arrays it spoils)
METRICS_FAULTS = {
    "mu_without_shift": ("1x75x43 noisy", {"part_ssim"}),
    "apron_owned_twice": ("1x75x43 noisy", {"part_ad", "part_sq"}),
    "pool_pad_behind": ("3x161x161 noisy", {"pool_bits", "pool"}),
}


def metrics_inputs(shape, family):
    x, y = MR.make_pair(shape, family)
    return x, y


def old_bars_metrics(x, y, want_ms, got):
    """Would tests/test_gpu_metrics.py's bars reject this result?  metrics_ref.tolerance(dev32) on the means, 1e-6 relative on l1 and
    the mean squared error."""
    import torch
    r64 = MR.image_metrics(x, y, clamp=False, ms_ssim=want_ms)
    r32 = MR.image_metrics(x, y, clamp=False, ms_ssim=want_ms, dtype=torch.float32)
    ok = ~np.isnan(r64["levels"])
    dev32 = max(np.abs(r32["levels"][ok] - r64["levels"][ok]).max(), abs(r32["out"][0, 2] - r64["out"][0, 2]))
    tol = MR.tolerance(dev32)
    o, lv = np.asarray(got["out"], np.float64), np.asarray(got["levels"], np.float64)
    dev = max(np.abs(lv[ok] - r64["levels"][ok]).max(), abs(o[0, 2] - r64["out"][0, 2]))
    return not bool(dev <= tol and abs(o[0, 0] / r64["out"][0, 0] - 1) <= 1e-6 and abs(o[0, 1] - r64["out"][0, 1]) <= 1e-4)
