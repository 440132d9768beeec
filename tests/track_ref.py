"""NumPy restatement of riggs_amd/track.py (csrc/track.hip; include/riggs_hip.h states both methods): the confidence-weighted
Gaussian window on SO(3) (the chordal L2 mean of Markley, Cheng, Crassidis & Oshman 2007) and the one-euro filter (Casiez, Roussel
& Vogel 2012) on unit quaternions and the root translation.

``dtype`` float64 is the oracle: its eigenvector comes from ``numpy.linalg.eigh``.  float32 is the yardstick for rounding: every
operation is rounded to float32, the sums run in the kernel's stated order (the window ascending) and the eigenvector comes from
the kernel's four cyclic Jacobi sweeps.  Which samples are valid is decided in float32 in both forms, as the kernel decides it.

Also the seeded generator of the test tracks and the list of cases, shared by the CPU and the GPU tests."""
from __future__ import annotations

import numpy as np

MAX_RADIUS, MAX_JOINTS, SWEEPS = 64, 256, 4
TWO_PI32 = np.float32(6.2831855)


def taps(sigma, radius=None):
    """(R, g (R + 1,) float32): exp(-d^2 / (2 sigma^2)) in float64, rounded once."""
    R = int(np.ceil(3.0 * float(sigma))) if radius is None else int(radius)
    d = np.arange(R + 1, dtype=np.float64)
    g = np.ones(R + 1) if R == 0 else np.exp(-(d * d) / (2.0 * float(sigma) * float(sigma)))
    return R, g.astype(np.float32)


def dot4(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def unit(q32, dtype):
    """(q / |q| in dtype, valid): valid iff 0 < |q|^2 < inf in float32; invalid rows come back as zeros."""
    with np.errstate(all="ignore"):
        n2 = dot4(q32, q32)
        ok = (n2 > 0) & (n2 < np.inf)
    q = np.where(ok[..., None], q32, np.float32(1.0)).astype(dtype)
    q = q / np.sqrt(dot4(q, q))[..., None]
    return np.where(ok[..., None], q, dtype(0)), ok


def confident(w32, shape):
    if w32 is None:
        return np.ones(shape, np.float32), np.ones(shape, bool)
    with np.errstate(invalid="ignore"):
        ok = np.asarray(w32, np.float32) > 0
    return np.where(ok, np.asarray(w32, np.float32), np.float32(0)), ok


def finite3(p32):
    with np.errstate(invalid="ignore"):
        return (np.abs(p32) < np.inf).all(-1)


def jacobi_dominant(m):
    """m (..., 4, 4) symmetric -> the normalised column of the largest diagonal entry after SWEEPS cyclic Jacobi sweeps, every
    operation in m's dtype (include/riggs_hip.h: riggs_track_smooth)."""
    T = m.dtype.type
    a = [[m[..., r, c].copy() for c in range(4)] for r in range(4)]
    v = [[np.full(m.shape[:-2], T(r == c), m.dtype) for c in range(4)] for r in range(4)]
    one, two, zero = T(1), T(2), T(0)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p in range(3):
                for q in range(p + 1, 4):
                    apq = a[p][q]
                    theta = (a[q][q] - a[p][p]) / (two * apq)
                    tt = one / (np.abs(theta) + np.sqrt(theta * theta + one))
                    t = np.where(apq != 0, np.where(theta < 0, -tt, tt), zero)
                    c = one / np.sqrt(t * t + one)
                    s = t * c
                    a[p][p] = a[p][p] - t * apq
                    a[q][q] = a[q][q] + t * apq
                    a[p][q] = a[q][p] = np.zeros_like(apq)
                    for r in range(4):
                        if r != p and r != q:
                            arp, arq = a[r][p], a[r][q]
                            a[r][p] = a[p][r] = c * arp - s * arq
                            a[r][q] = a[q][r] = s * arp + c * arq
                        vrp, vrq = v[r][p], v[r][q]
                        v[r][p] = c * vrp - s * vrq
                        v[r][q] = s * vrp + c * vrq
    best = a[0][0]
    out = [v[e][0] for e in range(4)]
    for k in range(1, 4):
        take = a[k][k] > best
        best = np.where(take, a[k][k], best)
        out = [np.where(take, v[e][k], out[e]) for e in range(4)]
    out = np.stack(out, -1)
    return out / np.sqrt(dot4(out, out))[..., None]


def smooth(rot, trans, sigma, radius=None, weights=None, trans_weights=None, wrap=False, dtype=np.float64, g=None):
    """rot (B, T, J, 4), trans (B, T, 3) or None, weights (B, T, J) or None, trans_weights (B, T) or None, all float32 ->
    dict(local_rotation, global_trans, support in ``dtype``; for float64 also ratio = lambda_2 / lambda_1, NaN without support)."""
    D = np.dtype(dtype).type
    R, g = taps(sigma, radius) if g is None else (int(radius), np.asarray(g, np.float32))  # (g: the taps as a launch receives them)
    rot = np.asarray(rot, np.float32)
    B, T, J = rot.shape[:3]
    if not 0 <= R <= MAX_RADIUS:
        raise ValueError("radius")
    if wrap and 2 * R + 1 > T:
        raise ValueError("wrap")
    q, qok = unit(rot, D)
    c, cok = confident(weights, (B, T, J))
    valid = qok & cok
    g, c = g.astype(D), c.astype(D)
    t = np.arange(T)
    M = np.zeros((B, T, J, 4, 4), D)
    sup = np.zeros((B, T, J), D)
    if trans is not None:
        trans = np.asarray(trans, np.float32)
        tc, tcok = confident(trans_weights, (B, T))
        tvalid = tcok & finite3(trans)
        p = np.where(tvalid[..., None], trans, np.float32(0)).astype(D)
        tc = tc.astype(D)
        acc, tsup = np.zeros((B, T, 3), D), np.zeros((B, T), D)
    for d in range(-R, R + 1):  # the window ascending
        s = t + d
        inside = np.ones(T, bool) if wrap else (s >= 0) & (s < T)
        s = s % T if wrap else np.clip(s, 0, T - 1)
        on = valid[:, s] & inside[None, :, None]
        wgt = g[abs(d)] * c[:, s]
        qs = q[:, s]
        sup = np.where(on, sup + wgt, sup)
        wq = wgt[..., None] * qs
        M = np.where(on[..., None, None], M + wq[..., :, None] * qs[..., None, :], M)
        if trans is not None:
            ton = tvalid[:, s] & inside[None, :]
            tw = g[abs(d)] * tc[:, s]
            tsup = np.where(ton, tsup + tw, tsup)
            acc = np.where(ton[..., None], acc + tw[..., None] * p[:, s], acc)
    up = np.triu_indices(4, 1)
    M[..., up[1], up[0]] = M[..., up[0], up[1]]  # (the kernel forms the 10 entries a <= b, (w q_a) q_b, and mirrors them)
    has = sup > 0
    ratio = None
    if D is np.float64:
        lam, vec = np.linalg.eigh(M)
        out = vec[..., :, 3]
        with np.errstate(all="ignore"):
            ratio = np.where(has, lam[..., 2] / lam[..., 3], np.nan)
    else:
        out = jacobi_dominant(M)
    # the sign: the centre sample's hemisphere where it is valid, else the first non-zero component positive
    lead = np.where(out[..., 0] != 0, out[..., 0], np.where(out[..., 1] != 0, out[..., 1], np.where(out[..., 2] != 0, out[..., 2], out[..., 3])))
    flip = np.where(valid, dot4(out, q) < 0, lead < 0)
    out = np.where(flip[..., None], -out, out)
    ident = np.array([1, 0, 0, 0], D)
    out = np.where(has[..., None], out, np.where(qok[..., None], q, ident))
    res = {"local_rotation": out, "support": np.where(has, sup, D(0)), "ratio": ratio, "global_trans": None}
    if trans is not None:
        with np.errstate(all="ignore"):
            res["global_trans"] = np.where((tsup > 0)[..., None], acc / tsup[..., None], trans.astype(D))
    return res


# ------------------------------------------------------------------------------------------------ one-euro
def fresh_state(B, J, dtype=np.float64):
    rot = np.zeros((B, J, 4), dtype)
    rot[..., 0] = 1
    return {"rotation": rot, "omega": np.zeros((B, J), dtype), "gap": np.full((B, J), -1, np.int32),
            "trans": np.zeros((B, 3), dtype), "velocity": np.zeros((B, 3), dtype), "trans_gap": np.full((B,), -1, np.int32)}


def one_euro(rot, trans, rate, min_cutoff=1.0, beta=0.0, d_cutoff=1.0, trans_min_cutoff=None, trans_beta=None, weights=None,
             trans_weights=None, state=None, dtype=np.float64):
    """rot (B, T, J, 4), trans (B, T, 3) or None -> dict(local_rotation, global_trans, state) in ``dtype``; the parameters are
    float32 values in both forms, as the kernel receives them."""
    D = np.dtype(dtype).type
    P = lambda x: D(np.float32(x))  # noqa: E731
    rate, fmin, beta, fd = P(rate), P(min_cutoff), P(beta), P(d_cutoff)
    tfmin = fmin if trans_min_cutoff is None else P(trans_min_cutoff)
    tbeta = beta if trans_beta is None else P(trans_beta)
    two_pi, one, two = D(TWO_PI32), D(1), D(2)
    rot = np.asarray(rot, np.float32)
    B, T, J = rot.shape[:3]
    x_all, qok = unit(rot, D)
    _, cok = confident(weights, (B, T, J))
    valid = qok & cok
    st = fresh_state(B, J, D) if state is None else {k: np.array(v, copy=True) for k, v in state.items()}
    f, om, gap = st["rotation"].astype(D), st["omega"].astype(D), st["gap"].copy()
    out = np.zeros((B, T, J, 4), D)

    def alpha(fc, dt):
        with np.errstate(divide="ignore"):
            return one / (one + one / ((two_pi * fc) * dt))

    with np.errstate(all="ignore"):
        for t in range(T):
            x, ok = x_all[:, t], valid[:, t]
            first = ok & (gap < 0)
            upd = ok & (gap >= 0)
            dt = (gap + 1).astype(D) / rate
            dot = dot4(x, f)
            x = np.where((dot < 0)[..., None], -x, x)
            dot = np.minimum(np.abs(dot), one)
            th = np.arccos(dot).astype(D)
            sn = np.sin(th).astype(D)
            speed = (two * th) / dt
            ad = alpha(fd, dt)
            om_new = ad * speed + (one - ad) * om
            al = alpha(fmin + beta * om_new, dt)
            lin = ~(sn > D(np.float32(1e-6)))
            w0 = np.where(lin, one - al, np.sin((one - al) * th).astype(D) / sn)
            w1 = np.where(lin, al, np.sin(al * th).astype(D) / sn)
            r = w0[..., None] * f + w1[..., None] * x
            r = r / np.sqrt(dot4(r, r))[..., None]
            f = np.where(first[..., None], x_all[:, t], np.where(upd[..., None], r, f))
            om = np.where(first, D(0), np.where(upd, om_new, om))
            gap = np.where(ok, 0, np.where(gap >= 0, gap + 1, gap)).astype(np.int32)
            out[:, t] = np.where((gap < 0)[..., None], np.array([1, 0, 0, 0], D), f)
    st["rotation"], st["omega"], st["gap"] = f, om, gap
    res = {"local_rotation": out, "global_trans": None, "state": st}
    if trans is not None:
        trans = np.asarray(trans, np.float32)
        _, tcok = confident(trans_weights, (B, T))
        tvalid = tcok & finite3(trans)
        p_all = np.where(tvalid[..., None], trans, np.float32(0)).astype(D)
        pf, v, tgap = st["trans"].astype(D), st["velocity"].astype(D), st["trans_gap"].copy()
        tout = np.zeros((B, T, 3), D)
        with np.errstate(all="ignore"):
            for t in range(T):
                p, ok = p_all[:, t], tvalid[:, t]
                first, upd = ok & (tgap < 0), ok & (tgap >= 0)
                dt = ((tgap + 1).astype(D) / rate)[:, None]
                ad = alpha(fd, dt)
                v_new = ad * ((p - pf) / dt) + (one - ad) * v
                speed = np.sqrt((v_new[:, 0] * v_new[:, 0] + v_new[:, 1] * v_new[:, 1]) + v_new[:, 2] * v_new[:, 2])[:, None]
                al = alpha(tfmin + tbeta * speed, dt)
                p_new = al * p + (one - al) * pf
                pf = np.where(first[:, None], p, np.where(upd[:, None], p_new, pf))
                v = np.where(first[:, None], D(0), np.where(upd[:, None], v_new, v))
                tgap = np.where(ok, 0, np.where(tgap >= 0, tgap + 1, tgap)).astype(np.int32)
                tout[:, t] = np.where((tgap < 0)[:, None], D(0), pf)
        st["trans"], st["velocity"], st["trans_gap"] = pf, v, tgap
        res["global_trans"] = tout
    return res


# ------------------------------------------------------------------------------------------------ measures
def rotation_angle(a, b):
    """The angle between the rotations of unit quaternions a and b, 2 acos |dot|, evaluated from the chord as 4 asin(|a -+ b| / 2)
    (the same angle; acos loses half its digits next to 1)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a / np.linalg.norm(a, axis=-1, keepdims=True), b / np.linalg.norm(b, axis=-1, keepdims=True)
    chord = np.minimum(np.linalg.norm(a - b, axis=-1), np.linalg.norm(a + b, axis=-1))
    return 4.0 * np.arcsin(np.minimum(chord / 2.0, 1.0))


def trans_extent(trans):
    """The largest axis range of the track's finite translations; 1 where that is 0."""
    p = np.asarray(trans, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(-1)]
    e = float((p.max(0) - p.min(0)).max()) if len(p) else 0.0
    return e if e > 0 else 1.0


# ------------------------------------------------------------------------------------------------ tracks and cases
def axis_angle_quat(axis, angle):
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    return np.concatenate([np.cos(angle / 2)[..., None], np.sin(angle / 2)[..., None] * axis], -1)


def quat_mul(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def make_track(B, T, J, seed, noise=0.6, step=0.15, gaps=0.2, loop=False):
    """Per joint: a random start rotation, a step of ``step`` rad about a random axis per frame, noise about a random axis with its
    angle uniform in [0, noise] rad, a random sign and a random scale in [0.5, 2] per sample; confidences uniform in [0.1, 1] with
    ``gaps`` of the samples set to 0.  The translation: a random walk with noise, the same confidences rule.  ``loop``: a looping
    clip, which is what ``wrap`` is for: the walk runs out to frame T // 2 and back the way it came, so frame T - 1 is next to frame 0.
    -> dict(rot (B,T,J,4), trans (B,T,3), weights (B,T,J), trans_weights (B,T)) float32, clean (B,T,J,4) float64 (before the noise)."""
    rng = np.random.default_rng(seed)
    q = np.zeros((B, T, J, 4))
    cur = rng.standard_normal((B, J, 4))
    cur /= np.linalg.norm(cur, axis=-1, keepdims=True)
    for t in range(T):
        if t:
            cur = quat_mul(cur, axis_angle_quat(rng.standard_normal((B, J, 3)), np.full((B, J), step)))
        q[:, t] = cur
    back = np.minimum(np.arange(T), T - np.arange(T)) if loop else np.arange(T)
    q = q[:, back]
    noisy = quat_mul(q, axis_angle_quat(rng.standard_normal((B, T, J, 3)), rng.uniform(0, noise, (B, T, J))))
    noisy *= (rng.choice([-1.0, 1.0], (B, T, J)) * rng.uniform(0.5, 2.0, (B, T, J)))[..., None]
    w = rng.uniform(0.1, 1.0, (B, T, J))
    w[rng.uniform(size=(B, T, J)) < gaps] = 0.0
    trans = np.cumsum(0.05 * rng.standard_normal((B, T, 3)), 1)[:, back] + 0.02 * rng.standard_normal((B, T, 3))
    tw = rng.uniform(0.1, 1.0, (B, T))
    tw[rng.uniform(size=(B, T)) < gaps] = 0.0
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return {"rot": f(noisy), "trans": f(trans), "weights": f(w), "trans_weights": f(tw), "clean": q}


SIGMA = {0: 1.0, 1: 0.7, 3: 1.0, 6: 2.0, 15: 5.0, 64: 21.0}


def _cases():
    out = []
    # clipping: T in {1, 2, R, R + 1, 2R + 1, 2R + 2} per R, wrap where 2R + 1 <= T
    for R in (0, 1, 6, 64):
        for T in sorted({1, 2, 2 * R + 1, 2 * R + 2} | ({R, R + 1} if R else set())):
            for wrap in (False, True):
                if not wrap or 2 * R + 1 <= T:
                    out.append(dict(B=1, T=T, J=24, R=R, wrap=wrap))
    # lanes: B T J in {1, 255, 256, 257, 3 * 256 + 5}; the joint counts; B = 3
    for B, T, J in ((1, 1, 1), (1, 255, 1), (3, 85, 1), (1, 256, 1), (1, 1, 256), (1, 257, 1), (1, 773, 1), (3, 14, 65), (3, 3, 256),
                    (3, 14, 24)):
        out.append(dict(B=B, T=T, J=J, R=6 if T >= 13 else 1, wrap=False))
    out.append(dict(B=3, T=14, J=24, R=6, wrap=True))
    # the sizes of the conditioning experiment
    for R in (3, 6, 15):
        out.append(dict(B=1, T=48, J=6, R=R, wrap=False))
    for n, c in enumerate(out):
        c.update(sigma=SIGMA[c["R"]], seed=1000 + n, name="b%d_t%d_j%d_r%d%s" % (c["B"], c["T"], c["J"], c["R"], "_wrap" if c["wrap"] else ""))
    return out


CASES = _cases()
_REFS = {}


def case_reference(case):
    """(track, float64 result, float32 result) of a case: computed once, shared, never changed."""
    if case["name"] not in _REFS:
        tr = make_track(case["B"], case["T"], case["J"], case["seed"], loop=case["wrap"])
        kw = dict(sigma=case["sigma"], radius=case["R"], weights=tr["weights"], trans_weights=tr["trans_weights"], wrap=case["wrap"])
        _REFS[case["name"]] = (tr, smooth(tr["rot"], tr["trans"], dtype=np.float64, **kw), smooth(tr["rot"], tr["trans"], dtype=np.float32, **kw))
    return _REFS[case["name"]]


EURO = dict(rate=30.0, min_cutoff=1.5, beta=0.4, d_cutoff=1.0, trans_min_cutoff=1.0, trans_beta=0.7)


def euro_track(B, J, seed, T=40):
    """A generated track with gaps at the first frame, in a run of 5 and at the last frame (every joint and the translation), on top
    of the generator's own."""
    tr = make_track(B, T, J, seed, noise=0.2)
    for k in ("weights", "trans_weights"):
        tr[k][:, 0] = 0
        tr[k][:, 20:25] = 0
        tr[k][:, T - 1] = 0
    return tr
