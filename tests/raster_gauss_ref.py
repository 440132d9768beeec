"""Float64 reference of the rasterizer's per-Gaussian stage (csrc/preprocess.hip: preprocess_fwd and the two launch forms of
preprocess_bwd, with gauss_math.h and color_job.h) and a per-element bound for every output.

The kernels are checked from the SAME fp32 inputs they read.  Three pieces live here:

``reference``   the per-Gaussian formulas in float64 torch, written with matrix algebra (view transform, perspective divide with
    its + 1e-7, Sigma3D = R S S R^T, the 2-D covariance J W Sigma W^T J^T with the 1.3 tan(fov) frustum clamp and the + 0.3
    low-pass, conic = inverse, radius 3 sqrt(lambda_max), SH colour + 0.5 clamped at 0, and the render glue: sigmoid, exp,
    normalize, the residuals d_xyz / d_rotation / d_scaling, the isotropic (N, 1) scaling).  Every gradient is float64 AUTOGRAD of
    those formulas applied to the cotangent record the compositing backward hands over (csrc/raster_internal.h,
    PreBwdArgs::gacc): dL/d(NDC x), dL/d(NDC y), dL/dA, dL/dB, dL/dC, dL/d opacity, dL/d rgb (3), dL/d depth, with A, B, C true
    partials of power = -0.5 (A dx^2 + C dy^2) - B dx dy.  No hand-derived gradient is shared with the kernel or with
    oracle/raster_ref.c: the derivatives of the constants (1e-7 of the divide, 0.3, the clamp) come out of autograd.  (The kernel
    computes the conic's backward with 1 / (det^2 + 1e-7) where the exact derivative has 1 / det^2: the reference has the exact
    one, and the bound carries the difference, 1e-7 / det^2 relative, through the kernel's steps like any other term.)

``kernel_steps``   the kernel's own steps, op by op, written ONCE over an abstract arithmetic.  With ``F32`` it is the float32
    restatement (torch float32 on the host rounds every operation once, as -ffp-contract=off with correctly rounded divide and
    square root does on the device), in a chosen evaluation order of every sum; its ``fault`` argument plants the errors that
    tests/test_raster_gauss_ref_cpu.py shows the bounds to reject.  With ``Bounded`` it is the error analysis:

``bounds``   a running first-order-plus-remainder error analysis of those steps.  Every quantity is a pair (v, e): v its float64
    value, e a bound of |fp32 value - v| for ANY fp32 evaluation of the same steps.  u = 2^-24.  The rules, each with the
    rounding of its own result, u (|v| + e), and TINY = 2^-149 where the result is not exactly zero (a result in the denormals):
        a +- b:   e_a + e_b
        a b:      |a| e_b + |b| e_a + e_a e_b                       (every product taken absolutely)
        a / b:    (e_a + |a / b| e_b) / (|b| - e_b)
        sqrt a:   e_a / (sqrt(a - e_a) + sqrt(a))
        sum of n terms in ANY order (``fsum``):  sum e_i + (n - 1) u sum (|t_i| + e_i)
        expf a:   v expm1(e_a) + (2 EXP_ULP + 2 |a|) u v + FLUSH     (EXP_ULP, FLUSH of tests/skin_ref.py; 2 |a| u: the scaling of
                  the argument to base 2); the sigmoid is 1 / (1 + expf(-x)) by the rules above
        max / min with a constant, the clamp: 1-Lipschitz, e passes through; a product with a power of two is exact
        a constant c of the source (0.3f, 1.3f, 1e-7f, the SH factors): v = c, e = |c - fp32(c)|
    Inputs are exact (e = 0).  The count of roundings on the longest path is therefore not a constant chosen here but the sum
    the rules produce, step by step along the kernel's own chain (e.g. a cov2D entry: the view transform's 4-term sums, the
    quotient t_x / t_z, J's two quotients, M2's 2-term sums, then two nested 3-term sums of products and the + 0.3f).  The
    longest chain, dL/drotations with the glue, is ~ 60 operations deep; on the GPU grid the kernels sit at 0.3 - 1.0 of their
    bounds (profiles/raster_gauss_parity.json).  The two cancelling quantities carry their own terms instead of a multiple of
    the result:
        det = a c - b^2:   e = |a| e_c + |c| e_a + 2 |b| e_b + u (a c + b^2) + ...: of order u (a c + b^2), however small det is;
        g - q (q . g) (the quaternion normalisation and the SH view direction):  e_g + |q| e_dot + |dot| e_q + u (|g| + |q dot|),
            with e_dot = sum_i (|q_i| e_g_i + |g_i| e_q_i) + 3 u sum |q_i g_i|: of the size of g, not of the projected result;
    and whatever follows (1 / det, the conic, 1 / (det^2 + 1e-7), the division by |v| or by the view distance) multiplies them by
    its own absolute partial derivative, which is what the rules above do.  The rotation gradient of an isotropic Gaussian is
    exactly zero in exact arithmetic: its v is ~ 1e-17 and its e is the rounding magnitude of the terms that cancel, nothing else.
    No constant was tuned on kernel output.

Exact zeros.  An element whose bound is 0 is compared exactly: the rows of a Gaussian without a record or with radius 0, the
third column of dL_dmeans2D, a clamped colour channel (its rgb and its share of dL/dsh), the SH coefficients above the active
degree, and the pass-through outputs (dL_dmeans2D, and with activated inputs / colors_precomp dL_dopacities / dL_dcolors_precomp),
which return the record's numbers bit for bit.

Decisions.  Visibility (radii > 0) and the clamp bits are the kernel's own where the caller has them; the frustum clamp is
recomputed in float64.  ``ambiguous`` marks every Gaussian on which a recomputed decision is within its own error bound (both
sides') of its threshold: |t_x / t_z| against 1.3 tan(fov x), the same in y, t_z against 0.2, a colour channel against 0.  The
tests admit none (tests/test_gpu_raster_gauss_f64.build asserts it on the host).  The radius is an integer: ``radius_sets``
gives ceil of both ends of 3 sqrt(lambda) -+ e; they differ only where the bound straddles an integer.

Pure torch on the CPU (N <= a few thousand)."""
import math

import numpy as np
import torch

from tests import dense_splat as DS
from tests.mlp_ref import assert_within, violations  # noqa: F401  (re-exported: the same checker)
from tests.skin_ref import EXP_ULP, FLUSH

U = 2.0 ** -24
TINY = 2.0 ** -149
NEAR_Z = 0.2
F64 = torch.float64

GRAD_KEYS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacities", "dL_dscales", "dL_drotations", "dL_dd_scaling", "dL_dcov3D", "dL_dsh",
             "dL_dsh_rest", "dL_dcolors_precomp")
FWD_KEYS = ("px", "py", "depth", "conic", "opacity", "rgb", "cov3D")
FAULTS = ("clamp_x_ignored", "clamped_colour_not_zeroed", "sh_dir_dropped", "sh_dir_no_projection", "d_scaling_not_in_s",
          "dd_scaling_times_exp", "raw_scaling_times_s", "quat_no_projection", "quat_div_one", "iso_column0", "dR_transposed",
          "conic_B_halved", "depth_row")


# ------------------------------------------------------------------------------------------------ the two arithmetics
class Er:
    """(v, e): a float64 value and a bound of what any fp32 evaluation of the same steps may differ from it."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def _rnd(v, e):
        e = e + U * (v.abs() + e)
        return Er(v, e + TINY * ((v.abs() + e) > 0))

    @staticmethod
    def _scalar(x):
        x = float(x)
        assert float(np.float32(x)) == x, "a literal of the kernel that fp32 does not hold: use const()"
        return x

    def __neg__(self):
        return Er(-self.v, self.e)

    def __add__(self, o):
        if not isinstance(o, Er):
            return Er._rnd(self.v + Er._scalar(o), self.e)
        return Er._rnd(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        if not isinstance(o, Er):
            return Er._rnd(self.v - Er._scalar(o), self.e)
        return Er._rnd(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Er._rnd(Er._scalar(o) - self.v, self.e)

    def __mul__(self, o):
        if not isinstance(o, Er):
            o = Er._scalar(o)
            m = abs(o)
            if m == 0.0 or math.frexp(m)[0] == 0.5:  # zero or a power of two: exact
                return Er(self.v * o, self.e * m)
            return Er._rnd(self.v * o, self.e * m)
        return Er._rnd(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    __rmul__ = __mul__

    @staticmethod
    def _div(av, ae, bv, be):
        v = av / bv
        room = bv.abs() - be
        e = torch.where(room > 0, (ae + v.abs() * be) / room.clamp_min(1e-300), torch.full_like(v, float("inf")))
        e = torch.where((ae == 0) & (be == 0), torch.zeros_like(e), e)
        return Er._rnd(v, e)

    def __truediv__(self, o):
        if not isinstance(o, Er):
            o = Er(torch.tensor(Er._scalar(o), dtype=F64))
        return Er._div(self.v, self.e, o.v, o.e)

    def __rtruediv__(self, o):
        o = torch.tensor(Er._scalar(o), dtype=F64)
        return Er._div(o, torch.zeros_like(o), self.v, self.e)


class Bounded:
    """The error analysis (see the module's docstring)."""
    name = "bounded"

    def inp(self, t):
        return Er(torch.as_tensor(t).to(F64))

    def const(self, x):
        x = float(x)
        return Er(torch.tensor(x, dtype=F64), torch.tensor(abs(x - float(np.float32(x))), dtype=F64))

    def val(self, x):
        return x.v

    def fsum(self, terms):
        v = terms[0].v
        e = terms[0].e
        s = terms[0].v.abs() + terms[0].e
        for t in terms[1:]:
            v = v + t.v
            e = e + t.e
            s = s + t.v.abs() + t.e
        e = e + (len(terms) - 1) * U * s
        return Er(v, e + TINY * (s > 0))

    def sqrt(self, x):
        v = torch.sqrt(x.v)
        lo = torch.sqrt((x.v - x.e).clamp_min(0.0))
        e = torch.where(x.e > 0, x.e / (lo + v).clamp_min(1e-300), torch.zeros_like(v))
        return Er._rnd(v, e)

    def exp(self, x):
        v = torch.exp(x.v)
        return Er(v, v * torch.expm1(x.e) + (2.0 * EXP_ULP + 2.0 * x.v.abs()) * U * v + FLUSH)

    def inv_det2(self, det):
        """The kernel's 1 / (det^2 + 1e-7f) as an approximation of the exact derivative's 1 / det^2: the difference is error."""
        x = 1.0 / (det * det + self.const(0.0000001))
        exact = 1.0 / (det.v * det.v)
        return Er(exact, x.e + (x.v - exact).abs())

    def maxc(self, x, c):
        return Er(x.v.clamp_min(c), x.e)

    def clamp(self, x, lim):  # clamp(x, -lim, lim), lim a 0-dim pair
        hit = x.v.abs() > lim.v
        return Er(torch.where(hit, torch.sign(x.v) * lim.v, x.v), torch.where(hit, lim.e.expand_as(x.e), x.e))

    def where(self, c, a, b):
        return Er(torch.where(c, a.v, b.v), torch.where(c, a.e, b.e))

    def zeros_like(self, x):
        return Er(torch.zeros_like(x.v))


class F32:
    """Plain float32: the restatement.  ``order``: 0 = every sum left to right (the kernel's), 1 = right to left, 2 = pairwise."""
    name = "f32"

    def __init__(self, order=0, dtype=torch.float32):
        self.order = order
        self.dtype = dtype

    def inp(self, t):
        return torch.as_tensor(t).to(self.dtype)

    def const(self, x):
        return torch.tensor(float(np.float32(x)), dtype=self.dtype)

    def val(self, x):
        return x.to(F64)

    def fsum(self, terms):
        terms = list(terms)
        if self.order == 1:
            terms = terms[::-1]
        if self.order == 2:
            while len(terms) > 1:
                terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
            return terms[0]
        s = terms[0]
        for t in terms[1:]:
            s = s + t
        return s

    def sqrt(self, x):
        return torch.sqrt(x)

    def inv_det2(self, det):
        return 1.0 / (det * det + self.const(0.0000001))

    def exp(self, x):
        return torch.exp(x)

    def maxc(self, x, c):
        return x.clamp_min(float(np.float32(c)))

    def clamp(self, x, lim):
        return torch.minimum(lim, torch.maximum(-lim, x))

    def where(self, c, a, b):
        return torch.where(c, a, b)

    def zeros_like(self, x):
        return torch.zeros_like(x)


def _val(x):
    return x.v if isinstance(x, Er) else x.to(F64)


def _err(x):
    return x.e if isinstance(x, Er) else torch.zeros_like(x, dtype=F64)


# ------------------------------------------------------------------------------------------------ the kernel's steps
def _quat_R(q):
    r, x, y, z = q
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y),
            2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
            2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)]


def _sh_basis(A, deg, x, y, z):
    c = A.const
    B = [c(DS.C0)]
    if deg > 0:
        B += [c(-DS.C1) * y, c(DS.C1) * z, c(-DS.C1) * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        B += [c(DS.C2[0]) * xy, c(DS.C2[1]) * yz, c(DS.C2[2]) * (2.0 * zz - xx - yy), c(DS.C2[3]) * xz, c(DS.C2[4]) * (xx - yy)]
    if deg > 2:
        B += [c(DS.C3[0]) * y * (3.0 * xx - yy), c(DS.C3[1]) * xy * z, c(DS.C3[2]) * y * (4.0 * zz - xx - yy),
              c(DS.C3[3]) * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), c(DS.C3[4]) * x * (4.0 * zz - xx - yy), c(DS.C3[5]) * z * (xx - yy),
              c(DS.C3[6]) * x * (xx - 3.0 * yy)]
    return B


def _sh_dir_grad(A, deg, x, y, z, w):
    """gauss_math.h: sh_dir_grad — the terms of each component in the kernel's order."""
    c = A.const
    g = [[], [], []]
    if deg > 0:
        g[1].append(c(-DS.C1) * w[1])
        g[2].append(c(DS.C1) * w[2])
        g[0].append(c(-DS.C1) * w[3])
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        C20, C21, C22, C23, C24 = (c(v) for v in DS.C2)
        g[0].append(C20 * y * w[4])
        g[1].append(C20 * x * w[4])
        g[1].append(C21 * z * w[5])
        g[2].append(C21 * y * w[5])
        g[0].append(C22 * -2.0 * x * w[6])
        g[1].append(C22 * -2.0 * y * w[6])
        g[2].append(C22 * 4.0 * z * w[6])
        g[0].append(C23 * z * w[7])
        g[2].append(C23 * x * w[7])
        g[0].append(C24 * 2.0 * x * w[8])
        g[1].append(C24 * -2.0 * y * w[8])
    if deg > 2:
        C30, C31, C32, C33, C34, C35, C36 = (c(v) for v in DS.C3)
        g[0].append(C30 * 6.0 * xy * w[9])
        g[1].append(C30 * (3.0 * xx - 3.0 * yy) * w[9])
        g[0].append(C31 * yz * w[10])
        g[1].append(C31 * xz * w[10])
        g[2].append(C31 * xy * w[10])
        g[0].append(C32 * -2.0 * xy * w[11])
        g[1].append(C32 * (4.0 * zz - xx - 3.0 * yy) * w[11])
        g[2].append(C32 * 8.0 * yz * w[11])
        g[0].append(C33 * -6.0 * xz * w[12])
        g[1].append(C33 * -6.0 * yz * w[12])
        g[2].append(C33 * (6.0 * zz - 3.0 * xx - 3.0 * yy) * w[12])
        g[0].append(C34 * (4.0 * zz - 3.0 * xx - yy) * w[13])
        g[1].append(C34 * -2.0 * xy * w[13])
        g[2].append(C34 * 8.0 * xz * w[13])
        g[0].append(C35 * 2.0 * xz * w[14])
        g[1].append(C35 * -2.0 * yz * w[14])
        g[2].append(C35 * (xx - yy) * w[14])
        g[0].append(C36 * (3.0 * xx - 3.0 * yy) * w[15])
        g[1].append(C36 * -6.0 * xy * w[15])
    return [A.fsum(t) if t else None for t in g]


def _cov2d(A, p, c6, V, fx, fy, tanx, tany):
    """gauss_math.h: cov2d_eval."""
    tx = A.fsum([V[0] * p[0], V[4] * p[1], V[8] * p[2], V[12]])
    ty = A.fsum([V[1] * p[0], V[5] * p[1], V[9] * p[2], V[13]])
    tz = A.fsum([V[2] * p[0], V[6] * p[1], V[10] * p[2], V[14]])
    limx, limy = A.const(1.3) * tanx, A.const(1.3) * tany
    txtz, tytz = tx / tz, ty / tz
    o = {"txtz": txtz, "tytz": tytz, "limx": limx, "limy": limy, "tz": tz}
    o["clamp_x"] = A.val(txtz).abs() > A.val(limx)
    o["clamp_y"] = A.val(tytz).abs() > A.val(limy)
    tx = A.clamp(txtz, limx) * tz
    ty = A.clamp(tytz, limy) * tz
    o["tx"], o["ty"] = tx, ty
    J00, J02 = fx / tz, -(fx * tx) / (tz * tz)
    J11, J12 = fy / tz, -(fy * ty) / (tz * tz)
    M2 = [J00 * V[0] + J02 * V[2], J00 * V[4] + J02 * V[6], J00 * V[8] + J02 * V[10],
          J11 * V[1] + J12 * V[2], J11 * V[5] + J12 * V[6], J11 * V[9] + J12 * V[10]]
    o["M2"] = M2
    s00 = A.fsum([c6[0] * M2[0], c6[1] * M2[1], c6[2] * M2[2]])
    s10 = A.fsum([c6[1] * M2[0], c6[3] * M2[1], c6[4] * M2[2]])
    s20 = A.fsum([c6[2] * M2[0], c6[4] * M2[1], c6[5] * M2[2]])
    s01 = A.fsum([c6[0] * M2[3], c6[1] * M2[4], c6[2] * M2[5]])
    s11 = A.fsum([c6[1] * M2[3], c6[3] * M2[4], c6[4] * M2[5]])
    s21 = A.fsum([c6[2] * M2[3], c6[4] * M2[4], c6[5] * M2[5]])
    o["a"] = A.fsum([M2[0] * s00, M2[1] * s10, M2[2] * s20]) + A.const(0.3)
    o["b"] = A.fsum([M2[0] * s01, M2[1] * s11, M2[2] * s21])
    o["c"] = A.fsum([M2[3] * s01, M2[4] * s11, M2[5] * s21]) + A.const(0.3)
    return o


def kernel_steps(A, t, cfg, rec=None, clamp_bits=None, fault=None, rec_err=None):
    """The steps of preprocess_fwd (and, with a record ``rec`` (N, 10), of preprocess_bwd's bwd_math + bwd_outputs) over the
    arithmetic ``A``.  ``t``: the case's CPU tensors (tests/test_gpu_raster_gauss_f64.build), ``cfg``: its dict.  ``clamp_bits``:
    the clamp bits the backward reads ((N,) uint8; default: the ones this forward computes).  ``fault``: one of FAULTS.
    ``rec_err`` (with the Bounded arithmetic): a bound (N, 10) of what the record the kernel reads may differ from ``rec`` — a record
    that is itself a computed quantity (tests/raster_comp_ref.py: the compositing backward's sums) instead of an injected one.
    Returns a dict of arithmetic values (lists per column); rows that are not visible hold garbage."""
    assert fault is None or fault in FAULTS
    glue, iso, deg, mod = cfg["glue"], cfg.get("iso", False), cfg["deg"], cfg.get("mod", 1.0)
    W, H = cfg["W"], cfg["H"]
    col = lambda x, n: [A.inp(x[:, j]) for j in range(n)]  # noqa: E731
    V = [A.inp(v) for v in t["view"].reshape(-1)]
    P = [A.inp(v) for v in t["proj"].reshape(-1)]
    cam = [A.inp(v) for v in t["campos"].reshape(-1)]
    tanx, tany, modv = A.inp(torch.tensor(np.float32(t["tanx"]))), A.inp(torch.tensor(np.float32(t["tany"]))), A.inp(torch.tensor(np.float32(mod)))
    o = {}
    # ---- finish_inputs
    p = col(t["means3D"], 3)
    if glue and t.get("d_xyz") is not None:
        dx = col(t["d_xyz"], 3)
        p = [p[j] + dx[j] for j in range(3)]
    raw_o = A.inp(t["opacities"].reshape(-1))
    op = 1.0 / (1.0 + A.exp(-raw_o)) if glue else raw_o
    need_sr = t.get("cov3D_precomp") is None
    es = s = q = vnorm = None
    if need_sr:
        if glue:
            if iso:
                e0 = A.exp(A.inp(t["scales"][:, 0]))
                es = [e0, e0, e0]
            else:
                es = [A.exp(x) for x in col(t["scales"], 3)]
            s = list(es)
            if t.get("d_scaling") is not None and fault != "d_scaling_not_in_s":
                ds = col(t["d_scaling"], 3)
                s = [s[j] + ds[j] for j in range(3)]
            v = col(t["rotations"], 4)
            if t.get("d_rotation") is not None:
                dr = col(t["d_rotation"], 4)
                v = [v[j] + dr[j] for j in range(4)]
            vnorm = A.maxc(A.sqrt(A.fsum([x * x for x in v])), 1e-12)
            q = [x / vnorm for x in v]
        else:
            s, q = col(t["scales"], 3), col(t["rotations"], 4)
    # ---- forward
    tzf = A.fsum([V[2] * p[0], V[6] * p[1], V[10] * p[2], V[14]])
    hx = A.fsum([P[0] * p[0], P[4] * p[1], P[8] * p[2], P[12]])
    hy = A.fsum([P[1] * p[0], P[5] * p[1], P[9] * p[2], P[13]])
    hw = A.fsum([P[3] * p[0], P[7] * p[1], P[11] * p[2], P[15]])
    pw = 1.0 / (hw + A.const(0.0000001))
    ndcx, ndcy = hx * pw, hy * pw
    if need_sr:
        Rm = _quat_R(q)
        s3 = [modv * s[j] for j in range(3)]
        Mm = [Rm[3 * r + j] * s3[j] for r in range(3) for j in range(3)]
        c6 = [A.fsum([Mm[3 * a + k] * Mm[3 * b + k] for k in range(3)]) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    else:
        c6 = col(t["cov3D_precomp"], 6)
    fx, fy = float(W) / (2.0 * tanx), float(H) / (2.0 * tany)
    cv = _cov2d(A, p, c6, V, fx, fy, tanx, tany)
    ca, cb, cc = cv["a"], cv["b"], cv["c"]
    det = ca * cc - cb * cb
    det_inv = 1.0 / det
    mid = 0.5 * (ca + cc)
    root = A.sqrt(A.maxc(mid * mid - det, 0.1))
    r3 = 3.0 * A.sqrt(mid + root)  # (lam1 = mid + root >= lam2)
    px = ((ndcx + 1.0) * float(W) - 1.0) * 0.5
    py = ((ndcy + 1.0) * float(H) - 1.0) * 0.5
    o.update(px=px, py=py, depth=tzf, conic=[cc * det_inv, -(cb * det_inv), ca * det_inv], opacity=op, cov3D=c6, r3=r3, cv=cv, det=det)
    rad = torch.ceil(_val(r3))
    pxv, pyv = _val(px), _val(py)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    f32t = lambda x: x.float().double()  # noqa: E731  (the rectangle is fp32 arithmetic on fp32 values)
    x0 = torch.trunc(f32t(f32t(pxv - rad) / 16)).clamp(0, gx)
    x1 = torch.trunc(f32t(f32t(f32t(pxv + rad) + 15) / 16)).clamp(0, gx)
    y0 = torch.trunc(f32t(f32t(pyv - rad) / 16)).clamp(0, gy)
    y1 = torch.trunc(f32t(f32t(f32t(pyv + rad) + 15) / 16)).clamp(0, gy)
    o["vis"] = (_val(tzf) > float(np.float32(NEAR_Z))) & (_val(det) != 0) & ((x1 - x0) * (y1 - y0) > 0)
    o["radius"] = torch.where(o["vis"], rad, torch.zeros_like(rad)).to(torch.int32)
    sh_mode = t.get("colors_precomp") is None
    M = 0
    if sh_mode:
        shs = t["shs"] if t.get("shs_rest") is None else torch.cat([t["shs"], t["shs_rest"]], 1)
        M = shs.shape[1]
        nb = (deg + 1) ** 2
        shv = [[A.inp(shs[:, k, c]) for c in range(3)] for k in range(M)]
        d = [p[j] - cam[j] for j in range(3)]
        ln = A.sqrt(A.fsum([x * x for x in d]))
        ud = [x / ln for x in d]
        Bk = _sh_basis(A, deg, *ud)
        pre = [A.fsum([Bk[k] * shv[k][c] for k in range(nb)]) + 0.5 for c in range(3)]
        o["rgb_pre"] = pre
        o["rgb"] = [A.maxc(x, 0.0) for x in pre]
        o["clamped"] = torch.stack([_val(x) < 0 for x in pre], 1)
    else:
        o["rgb"] = col(t["colors_precomp"], 3)
        o["clamped"] = torch.zeros(t["means3D"].shape[0], 3, dtype=torch.bool)
    if rec is None:
        return o
    # ---- bwd_math
    cl = o["clamped"] if clamp_bits is None else torch.stack([(clamp_bits.long() >> c) & 1 for c in range(3)], 1).bool()
    g = col(rec, 10)
    if rec_err is not None:
        g = [Er(x.v, rec_err[:, j].to(F64)) for j, x in enumerate(g)]
    g2x, g2y, gA, gB, gC, g_op, gd = g[0], g[1], g[2], g[3], g[4], g[5], g[9]
    gcol = g[6:9]
    if fault == "conic_B_halved":
        gB = 0.5 * gB
    d2inv = A.inv_det2(det)
    dL_da = d2inv * A.fsum([(-cc * cc) * gA, (cb * cc) * gB, -((cb * cb) * gC)])
    dL_db = d2inv * A.fsum([(2.0 * cb * cc) * gA, -((det + 2.0 * cb * cb) * gB), (2.0 * ca * cb) * gC])
    dL_dc = d2inv * A.fsum([(-cb * cb) * gA, (ca * cb) * gB, -((ca * ca) * gC)])
    M2 = cv["M2"]
    hb = 0.5 * dL_db
    DM = [None] * 6
    for j in range(3):
        DM[j] = dL_da * M2[j] + hb * M2[3 + j]
        DM[3 + j] = hb * M2[j] + dL_dc * M2[3 + j]
    GS = [M2[r] * DM[j] + M2[3 + r] * DM[3 + j] for r in range(3) for j in range(3)]
    S = [c6[0], c6[1], c6[2], c6[1], c6[3], c6[4], c6[2], c6[4], c6[5]]
    dM2 = [2.0 * A.fsum([DM[3 * r] * S[j], DM[3 * r + 1] * S[3 + j], DM[3 * r + 2] * S[6 + j]]) for r in range(2) for j in range(3)]
    dJ00 = A.fsum([dM2[0] * V[0], dM2[1] * V[4], dM2[2] * V[8]])
    dJ02 = A.fsum([dM2[0] * V[2], dM2[1] * V[6], dM2[2] * V[10]])
    dJ11 = A.fsum([dM2[3] * V[1], dM2[4] * V[5], dM2[5] * V[9]])
    dJ12 = A.fsum([dM2[3] * V[2], dM2[4] * V[6], dM2[5] * V[10]])
    tz = 1.0 / cv["tz"]
    tz2 = tz * tz
    tz3 = tz2 * tz
    zero = A.zeros_like(tz)
    dtx = (-fx) * tz2 * dJ02
    if fault != "clamp_x_ignored":
        dtx = A.where(cv["clamp_x"], zero, dtx)
    dty = A.where(cv["clamp_y"], zero, (-fy) * tz2 * dJ12)
    dtz = A.fsum([(-fx) * tz2 * dJ00, -(fy * tz2 * dJ11), (2.0 * fx * cv["tx"]) * tz3 * dJ02, (2.0 * fy * cv["ty"]) * tz3 * dJ12])
    mw = 1.0 / (hw + A.const(0.0000001))
    mul1, mul2 = hx * mw * mw, hy * mw * mw
    gm = []
    for j in range(3):
        terms = [V[4 * j] * dtx, V[4 * j + 1] * dty, V[4 * j + 2] * dtz,
                 (P[4 * j] * mw - P[4 * j + 3] * mul1) * g2x + (P[4 * j + 1] * mw - P[4 * j + 3] * mul2) * g2y,
                 (V[8 + j] if fault == "depth_row" else V[4 * j + 2]) * gd]
        gm.append(terms)
    g_sh = None
    if sh_mode:
        gcs = [gcol[c] if fault == "clamped_colour_not_zeroed" else A.where(cl[:, c], zero, gcol[c]) for c in range(3)]
        if deg > 0 and fault != "sh_dir_dropped":
            w = [A.fsum([shv[k][c] * gcs[c] for c in range(3)]) for k in range(nb)]
            gdir = _sh_dir_grad(A, deg, ud[0], ud[1], ud[2], w)
            dot = A.fsum([ud[j] * gdir[j] for j in range(3)])
            for j in range(3):
                gm[j].append((gdir[j] if fault == "sh_dir_no_projection" else gdir[j] - ud[j] * dot) / ln)
        g_sh = [[Bk[k] * gcs[c] if k < nb else zero for c in range(3)] for k in range(M)]
    gm = [A.fsum(terms) for terms in gm]
    out = {"dL_dmeans3D": gm, "dL_dmeans2D": [g2x, g2y, zero]}
    if sh_mode:
        if t.get("shs_rest") is None:
            out["dL_dsh"] = g_sh
        else:
            out["dL_dsh"], out["dL_dsh_rest"] = g_sh[:1], g_sh[1:]
    else:
        out["dL_dcolors_precomp"] = gcol
    gs = gq = None
    if not need_sr:
        out["dL_dcov3D"] = [GS[0], 2.0 * GS[1], 2.0 * GS[2], GS[4], 2.0 * GS[5], GS[8]]
    else:
        dMm = [2.0 * A.fsum([GS[3 * r] * Mm[j], GS[3 * r + 1] * Mm[3 + j], GS[3 * r + 2] * Mm[6 + j]]) for r in range(3) for j in range(3)]
        gs = [modv * A.fsum([Rm[j] * dMm[j], Rm[3 + j] * dMm[3 + j], Rm[6 + j] * dMm[6 + j]]) for j in range(3)]
        dR = [s3[j] * dMm[3 * r + j] for r in range(3) for j in range(3)]
        if fault == "dR_transposed":
            dR = [dR[3 * j + r] for r in range(3) for j in range(3)]
        r_, x, y, z = q
        gq = [2.0 * A.fsum([-(z * dR[1]), y * dR[2], z * dR[3], -(x * dR[5]), -(y * dR[6]), x * dR[7]]),
              2.0 * A.fsum([y * dR[1], z * dR[2], y * dR[3], -(2.0 * x * dR[4]), -(r_ * dR[5]), z * dR[6], r_ * dR[7], -(2.0 * x * dR[8])]),
              2.0 * A.fsum([-(2.0 * y * dR[0]), x * dR[1], r_ * dR[2], x * dR[3], z * dR[5], -(r_ * dR[6]), z * dR[7], -(2.0 * y * dR[8])]),
              2.0 * A.fsum([-(2.0 * z * dR[0]), -(r_ * dR[1]), x * dR[2], r_ * dR[3], -(2.0 * z * dR[4]), y * dR[5], x * dR[6], y * dR[7]])]
    # ---- bwd_outputs
    if glue:
        out["dL_dopacities"] = [g_op * op * (1.0 - op)]
        if need_sr:
            mulby = s if fault == "raw_scaling_times_s" else es
            if iso:
                out["dL_dscales"] = [gs[0] * mulby[0] if fault == "iso_column0" else A.fsum([gs[j] * mulby[j] for j in range(3)])]
            else:
                out["dL_dscales"] = [gs[j] * mulby[j] for j in range(3)]
            out["dL_dd_scaling"] = [gs[j] * es[j] for j in range(3)] if fault == "dd_scaling_times_exp" else list(gs)
            if fault == "quat_no_projection":
                out["dL_drotations"] = [gq[j] / vnorm for j in range(4)]
            else:
                dot = A.fsum([q[j] * gq[j] for j in range(4)])
                out["dL_drotations"] = [(gq[j] - q[j] * dot) if fault == "quat_div_one" else (gq[j] - q[j] * dot) / vnorm for j in range(4)]
    else:
        out["dL_dopacities"] = [g_op]
        if need_sr:
            out["dL_dscales"], out["dL_drotations"] = gs, gq
    o["grads"] = out
    return o


def _stack(cols, part):
    """A list (or list of lists) of arithmetic values -> one float64 tensor (N, ...) of their values / error bounds."""
    if isinstance(cols[0], list):
        return torch.stack([_stack(c, part) for c in cols], 1)
    return torch.stack([torch.broadcast_to(part(c), part(cols[0]).shape) for c in cols], 1)


def collect(o, with_record, sel, part=_val):
    """kernel_steps' result as plain tensors: forward arrays, and gradient arrays with every row outside ``sel`` exactly 0."""
    r = {"px": part(o["px"]), "py": part(o["py"]), "depth": part(o["depth"]), "conic": _stack(o["conic"], part), "opacity": part(o["opacity"]),
         "rgb": _stack(o["rgb"], part), "cov3D": _stack(o["cov3D"], part), "r3": part(o["r3"])}
    if with_record:
        for k, v in o["grads"].items():
            a = _stack(v, part)
            m = sel.reshape((-1,) + (1,) * (a.dim() - 1))
            r[k] = torch.where(m, a, torch.zeros_like(a))
    return r


# ------------------------------------------------------------------------------------------------ float64 reference
def _leaves(t, cfg):
    d = lambda k: None if t.get(k) is None else t[k].to(F64).clone().requires_grad_(True)  # noqa: E731
    Lf = {k: d(k) for k in ("means3D", "opacities", "scales", "rotations", "cov3D_precomp", "shs", "shs_rest", "colors_precomp", "d_xyz",
                            "d_rotation", "d_scaling")}
    if cfg["glue"] and Lf["cov3D_precomp"] is None and Lf["d_scaling"] is None:
        # (dL_dd_scaling may be asked for without a d_scaling input: the kernel writes dL/ds all the same — a zero residual here)
        Lf["d_scaling"] = torch.zeros(t["means3D"].shape[0], 3, dtype=F64, requires_grad=True)
    return Lf


def forward64(Lf, t, cfg):
    """The per-Gaussian outputs in float64 from the leaves ``Lf`` (differentiable): ndc (N, 2), depth, conic (N, 3), opacity, rgb
    (N, 3) before the clamp at 0, and Sigma3D (N, 6), 3 sqrt(lambda), the pixel centre."""
    glue, iso, deg, mod = cfg["glue"], cfg.get("iso", False), cfg["deg"], float(np.float32(cfg.get("mod", 1.0)))
    W, H = cfg["W"], cfg["H"]
    view, proj, campos = t["view"].to(F64), t["proj"].to(F64), t["campos"].to(F64)
    tanx, tany = float(np.float32(t["tanx"])), float(np.float32(t["tany"]))
    p = Lf["means3D"]
    if glue and Lf["d_xyz"] is not None:
        p = p + Lf["d_xyz"]
    N = p.shape[0]
    op = torch.sigmoid(Lf["opacities"].reshape(-1)) if glue else Lf["opacities"].reshape(-1)
    ph = torch.cat([p, torch.ones(N, 1, dtype=F64)], 1)
    pv, hom = ph @ view, ph @ proj
    ndc = hom[:, :2] / (hom[:, 3:4] + 1e-7)
    tz = pv[:, 2]
    if Lf["cov3D_precomp"] is None:
        if glue:
            sc = torch.exp(Lf["scales"])
            if iso:
                sc = sc.expand(N, 3)
            if Lf["d_scaling"] is not None:
                sc = sc + Lf["d_scaling"]
            v = Lf["rotations"] if Lf["d_rotation"] is None else Lf["rotations"] + Lf["d_rotation"]
            q = v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)
        else:
            sc, q = Lf["scales"], Lf["rotations"]
        Mm = DS.quat_R(q) * (mod * sc)[:, None, :]
        Sigma = Mm @ Mm.transpose(1, 2)
    else:
        Sigma = Lf["cov3D_precomp"][:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(N, 3, 3)
    fx, fy = W / (2 * tanx), H / (2 * tany)
    limx, limy = 1.3 * tanx, 1.3 * tany
    txtz, tytz = pv[:, 0] / tz, pv[:, 1] / tz
    cx, cy = txtz.detach().abs() > limx, tytz.detach().abs() > limy
    tx = torch.where(cx, (txtz.clamp(-limx, limx) * tz).detach(), pv[:, 0])
    ty = torch.where(cy, (tytz.clamp(-limy, limy) * tz).detach(), pv[:, 1])
    zero = torch.zeros_like(tz)
    Jm = torch.stack([fx / tz, zero, -fx * tx / tz ** 2, zero, fy / tz, -fy * ty / tz ** 2], -1).reshape(N, 2, 3)
    M2 = Jm @ view[:3, :3].T
    cov2 = M2 @ Sigma @ M2.transpose(1, 2)
    a, b, c = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], 1)
    mid = 0.5 * (a + c)
    r3 = 3 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1)))
    if Lf["colors_precomp"] is None:
        shs = Lf["shs"] if Lf["shs_rest"] is None else torch.cat([Lf["shs"], Lf["shs_rest"]], 1)
        sh16 = torch.cat([shs, torch.zeros(N, 16 - shs.shape[1], 3, dtype=F64)], 1) if shs.shape[1] < 16 else shs
        d = p - campos[None]
        rgb = DS.eval_sh(deg, sh16, d / d.norm(dim=1, keepdim=True)) + 0.5
    else:
        rgb = Lf["colors_precomp"]
    Sg = Sigma.detach()
    return {"ndc": ndc, "depth": tz, "conic": conic, "opacity": op, "rgb_pre": rgb, "r3": r3.detach(),
            "cov3D": torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1),
            "px": (((ndc[:, 0] + 1) * W - 1) * 0.5).detach(), "py": (((ndc[:, 1] + 1) * H - 1) * 0.5).detach(),
            "clamp_x": cx, "clamp_y": cy}


def reference(t, cfg, rec=None, vis=None, clamp_bits=None):
    """Forward values, and with a record the gradients: float64 autograd of ``forward64`` contracted with ``rec`` (N, 10) on the rows
    ``vis`` (the kernel's radii > 0) that hold a record, the clamped channels (``clamp_bits``, (N,) uint8: the kernel's own) cut off."""
    Lf = _leaves(t, cfg)
    f = forward64(Lf, t, cfg)
    sh_mode = t.get("colors_precomp") is None
    pre = f["rgb_pre"].detach()
    out = {k: f[k].detach() for k in ("px", "py", "depth", "conic", "opacity", "cov3D", "r3", "clamp_x", "clamp_y")}
    out["clamped"] = (pre < 0) if sh_mode else torch.zeros_like(pre, dtype=torch.bool)
    out["rgb"] = pre.clamp_min(0.0) if sh_mode else pre
    out["rgb_pre"] = pre
    if rec is None:
        return out
    N = pre.shape[0]
    rec = rec.to(F64)
    sel = vis & (rec != 0).any(1)
    cl = out["clamped"] if clamp_bits is None else torch.stack([(clamp_bits.long() >> c) & 1 for c in range(3)], 1).bool()
    keep = ~cl if sh_mode else torch.ones_like(cl)
    m = sel.to(F64)
    safe = lambda x: torch.where(sel.reshape((-1,) + (1,) * (x.dim() - 1)), x, torch.zeros_like(x))  # noqa: E731
    loss = ((safe(f["ndc"]) * rec[:, 0:2]).sum() + (safe(f["conic"]) * rec[:, 2:5]).sum() + (safe(f["opacity"]) * rec[:, 5]).sum()
            + (safe(f["rgb_pre"]) * rec[:, 6:9] * keep).sum() + (safe(f["depth"]) * rec[:, 9]).sum())
    names = [k for k, v in Lf.items() if v is not None]
    gr = dict(zip(names, torch.autograd.grad(loss, [Lf[k] for k in names], allow_unused=True)))
    z = lambda k: torch.zeros_like(Lf[k]) if gr.get(k) is None else torch.nan_to_num(gr[k]) * m.reshape((-1,) + (1,) * (Lf[k].dim() - 1))  # noqa: E731
    g = {"dL_dmeans3D": z("means3D"), "dL_dopacities": z("opacities").reshape(N, 1),
         "dL_dmeans2D": torch.cat([rec[:, 0:2] * m[:, None], torch.zeros(N, 1, dtype=F64)], 1)}
    if Lf["cov3D_precomp"] is None:
        g["dL_dscales"], g["dL_drotations"] = z("scales"), z("rotations")
        if cfg["glue"]:
            g["dL_dd_scaling"] = z("d_scaling")
    else:
        g["dL_dcov3D"] = z("cov3D_precomp")
    if sh_mode:
        g["dL_dsh"] = z("shs")
        if Lf["shs_rest"] is not None:
            g["dL_dsh_rest"] = z("shs_rest")
    else:
        g["dL_dcolors_precomp"] = z("colors_precomp")
    out["grads"] = g
    out["sel"] = sel
    return out


# ------------------------------------------------------------------------------------------------ bounds
def bounds(t, cfg, rec=None, vis=None, clamp_bits=None, rec_err=None):
    """(values, error bounds, ambiguous) of the kernel's steps: ``values`` the float64 evaluation of the kernel's own formulas (a
    second opinion of ``reference``), ``error bounds`` per element as the module's docstring derives them; exact-zero rules applied.
    ``ambiguous`` (N,) bool: a recomputed decision within its error of its threshold."""
    A = Bounded()
    with torch.no_grad():
        o = kernel_steps(A, t, cfg, rec=rec, clamp_bits=clamp_bits, rec_err=rec_err)
        sel = None
        if rec is not None:
            sel = vis & (rec != 0).any(1)
        val, err = collect(o, rec is not None, sel, _val), collect(o, rec is not None, sel, _err)
    cv = o["cv"]
    amb = ((cv["txtz"].v.abs() - cv["limx"].v).abs() <= cv["txtz"].e + cv["limx"].e) | \
          ((cv["tytz"].v.abs() - cv["limy"].v).abs() <= cv["tytz"].e + cv["limy"].e) | \
          ((cv["tz"].v - NEAR_Z).abs() <= cv["tz"].e + abs(NEAR_Z - float(np.float32(NEAR_Z))))
    if "rgb_pre" in o:
        amb = amb | torch.stack([x.v.abs() <= x.e for x in o["rgb_pre"]], 1).any(1)
        cl = o["clamped"] if clamp_bits is None else torch.stack([(clamp_bits.long() >> c) & 1 for c in range(3)], 1).bool()
        err["rgb"] = torch.where(cl, torch.zeros_like(err["rgb"]), err["rgb"])
    near = (cv["tz"].v - NEAR_Z).abs() <= cv["tz"].e + abs(NEAR_Z - float(np.float32(NEAR_Z)))
    amb = near | (amb & (cv["tz"].v > NEAR_Z))  # (behind the near plane nothing else is decided)
    if rec is not None:
        # pass-through outputs: the record's numbers bit for bit
        for k in ("dL_dmeans2D", "dL_dcolors_precomp") + (() if cfg["glue"] else ("dL_dopacities",)):
            if k in err and rec_err is None:  # (with ``rec_err`` they carry the record's own bound)
                err[k] = torch.zeros_like(err[k])
        for k in GRAD_KEYS:
            if k in err:
                err[k] = torch.nan_to_num(err[k], nan=float("inf"))
    return val, err, amb


def radius_sets(r3, e):
    """(lowest, highest) integer radius that 3 sqrt(lambda) = r3 -+ e admits."""
    return torch.ceil(r3 - e), torch.ceil(r3 + e)


def vacuity(ref, bnd):
    """The share of counted elements (bound > 0) whose bound is at least |reference|."""
    counted = bnd > 0
    n = int(counted.sum())
    return (float(((bnd >= ref.abs()) & counted).sum()) / n) if n else 0.0
