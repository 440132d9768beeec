"""NumPy restatement of the IK iteration of riggs_amd/pose_edit.py::solve_ik (csrc/ik.hip): damped least squares (Wampler 1986)
with Buss & Kim's clamping of the target step, on the rig's own kinematics (skeleton_utils/skeleton_warp.py:242-273: joint j's
quaternion turns joint j about its PARENT's rest position, the root about itself).  ``dtype`` float64 is the oracle; float32 is the
yardstick for rounding: every operation is rounded to ``dtype``, in the order the text of the method gives.

Also the generators of the test cases (random trees, poses, reachable targets), shared by the CPU and the GPU tests."""
from __future__ import annotations

import numpy as np

MAX_E, MAX_J = 8, 256


def quat_to_R(q):
    """utils/time_utils.py:115-132 with two_s = 2 / |q|^2."""
    r, i, j, k = q
    two_s = q.dtype.type(2.0) / (r * r + i * i + j * j + k * k)
    one = q.dtype.type(1.0)
    return np.array([[one - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r)],
                     [two_s * (i * j + k * r), one - two_s * (i * i + k * k), two_s * (j * k - i * r)],
                     [two_s * (i * k - j * r), two_s * (j * k + i * r), one - two_s * (i * i + j * j)]], dtype=q.dtype)


def quat_mul(a, b):
    """Hamilton product a (x) b, wxyz."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dtype=a.dtype)


def vparents(parents):
    p = np.asarray(parents, np.int64).copy()
    p[0] = 0
    return p


def fk(joints, parents, q, gt):
    """(R (J,3,3), t (J,3), posed (J,3)): G_j = G_vp(j) T_j, T_j = [R_j | c - R_j c] with c = joints[vp(j)], posed_j = G_j [x_j; 1] + gt."""
    J, vp = len(joints), vparents(parents)
    R, t = np.zeros((J, 3, 3), joints.dtype), np.zeros((J, 3), joints.dtype)
    for j in range(J):
        Rl = quat_to_R(q[j])
        c = joints[vp[j]]
        tl = c - Rl @ c
        if j == 0:
            R[j], t[j] = Rl, tl
        else:
            R[j], t[j] = R[vp[j]] @ Rl, R[vp[j]] @ tl + t[vp[j]]
    posed = np.einsum("jrc,jc->jr", R, joints) + t + gt
    return R, t, posed


def paths(parents, handles):
    """(E, J) bool: joint a is on the path root .. handle e, the handle's joint included."""
    vp = vparents(parents)
    on = np.zeros((len(handles), len(vp)), bool)
    for e, h in enumerate(handles):
        a = int(h)
        while True:
            on[e, a] = True
            if a == 0:
                break
            a = int(vp[a])
    return on


def cross_matrix(p):
    z = p.dtype.type(0)
    return np.array([[z, -p[2], p[1]], [p[2], z, -p[0]], [-p[1], p[0], z]], dtype=p.dtype)


def cholesky_solve(A, r):
    """A y = r by Cholesky (left-looking, column by column) and the two triangular solves (column-oriented)."""
    n = len(r)
    L = np.zeros_like(A)
    for k in range(n):
        v = A[k:, k].copy()
        for m in range(k):
            v = v - L[k:, m] * L[k, m]
        lkk = np.sqrt(v[0])
        L[k:, k] = v / lkk
        L[k, k] = lkk
    b = r.copy()
    for k in range(n):
        b[k] = b[k] / L[k, k]
        b[k + 1:] = b[k + 1:] - L[k + 1:, k] * b[k]
    for k in range(n - 1, -1, -1):
        b[k] = b[k] / L[k, k]
        b[:k] = b[:k] - L[k, :k] * b[k]
    return b


def extent_of(joints):
    """The largest axis range of the rest joints in float32 (the library's arithmetic); 1 where that is 0 (a single joint)."""
    j = np.asarray(joints, np.float32)
    e = np.float32((j.max(0) - j.min(0)).max())
    return e if e > 0 else np.float32(1.0)


def solve(joints, parents, q, gt, handles, targets, weights=None, locked=None, iterations=16, damping=None, max_step=None,
          solve_translation=False, dtype=np.float64, snapshots=None):
    """One problem.  -> dict(local_rotation (J,4), global_trans (3,), d_nodes (J,3), residual (E,)) in ``dtype``; with
    ``snapshots`` (iteration counts <= iterations) a dict of those, one per count: what a run of that many iterations returns."""
    T = np.dtype(dtype).type
    ext = extent_of(joints)
    damping = T(np.float32(0.05) * ext) if damping is None else T(np.float32(damping))
    max_step = T(np.float32(0.5) * ext) if max_step is None else T(np.float32(max_step))
    joints = np.asarray(joints, np.float32).astype(dtype)
    q = np.asarray(q, np.float32).astype(dtype).copy()
    gt = np.asarray(gt, np.float32).astype(dtype).reshape(3).copy()
    targets = np.asarray(targets, np.float32).astype(dtype)
    handles = np.asarray(handles, np.int64)
    J, E = len(joints), len(handles)
    w = np.ones(E, dtype) if weights is None else np.asarray(weights, np.float32).astype(dtype)
    locked = np.zeros(J, bool) if locked is None else np.asarray(locked, bool)
    vp = vparents(parents)
    live = w > 0
    s = np.where(live, np.sqrt(np.where(live, w, 1)), 0).astype(dtype)
    on = paths(parents, handles) & live[:, None] & ~locked[None, :]
    def result():
        posed = fk(joints, parents, q, gt)[2]
        res = np.sqrt(((targets - posed[handles]) ** 2).sum(-1))
        return {"local_rotation": q.copy(), "global_trans": gt.copy(), "d_nodes": posed, "residual": res}
    snaps = {}
    for it in range(iterations):
        if snapshots is not None and it in snapshots:
            snaps[it] = result()
        R, t, posed = fk(joints, parents, q, gt)
        piv = posed[vp]
        r = np.zeros(3 * E, dtype)
        Jm = np.zeros((3 * E, 3 * J + 3), dtype)
        P = np.zeros((E, J, 3), dtype)
        for e in range(E):
            if not live[e]:
                continue
            d = targets[e] - posed[handles[e]]
            n = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            if n > max_step:
                d = d * (max_step / n)
            r[3 * e:3 * e + 3] = s[e] * d
            for a in range(J):
                if on[e, a]:
                    P[e, a] = posed[handles[e]] - piv[a]
                    Jm[3 * e:3 * e + 3, 3 * a:3 * a + 3] = -s[e] * cross_matrix(P[e, a])
            if solve_translation:
                Jm[3 * e:3 * e + 3, 3 * J:] = s[e] * np.eye(3, dtype=dtype)
        A = Jm @ Jm.T + damping * damping * np.eye(3 * E, dtype=dtype)
        y = cholesky_solve(A.astype(dtype), r)
        for a in range(J):
            om = np.zeros(3, dtype)
            for e in range(E):
                if on[e, a]:
                    om = om + s[e] * np.cross(P[e, a], y[3 * e:3 * e + 3])
            delta = om if a == 0 else R[vp[a]].T @ om
            th = np.sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2])
            if th > 0:
                half = T(0.5) * th
                dq = np.concatenate([[np.cos(half)], (np.sin(half) / th) * delta]).astype(dtype)
                q[a] = quat_mul(dq, q[a])
        if solve_translation:
            dgt = np.zeros(3, dtype)
            for e in range(E):
                if live[e]:
                    dgt = dgt + s[e] * y[3 * e:3 * e + 3]
            gt = gt + dgt
    if snapshots is not None:
        if iterations in snapshots:
            snaps[iterations] = result()
        return snaps
    return result()


# --------------------------------------------------------------------------- the cases of the tests
def tree(J, seed, chain=False):
    """parents[i] = randint(0, i) (a straight chain: i - 1), bone offsets N(0, 0.25^2): (joints (J,3) float32, parents (J,) int32, -1 at the root)."""
    rng = np.random.default_rng(seed)
    parents = np.full(J, -1, np.int32)
    joints = np.zeros((J, 3), np.float32)
    joints[0] = rng.normal(0, 0.25, 3)
    for i in range(1, J):
        parents[i] = i - 1 if chain else rng.integers(0, i)
        off = np.array([0.25, 0, 0]) if chain else rng.normal(0, 0.25, 3)
        joints[i] = joints[parents[i]] + off
    return joints, parents


def depths(parents):
    d = np.zeros(len(parents), np.int64)
    for i in range(1, len(parents)):
        d[i] = d[parents[i]] + 1
    return d


def deepest(parents, E):
    """The E deepest joints (ties: the higher index first)."""
    d = depths(parents)
    return np.array(sorted(range(len(parents)), key=lambda i: (-d[i], -i))[:E], np.int32)


def pose(J, sigma, rng):
    q = np.zeros((J, 4), np.float32)
    q[:, 0] = 1
    return (q + rng.normal(0, sigma, (J, 4))).astype(np.float32)


# name -> (J, E, chain, solve_translation, seed)
CASES = {
    "root_only": (1, 1, False, True, 11),
    "two_joints": (2, 1, False, False, 12),
    "chain4": (4, 1, True, False, 13),
    "tree8": (8, 2, False, False, 20),
    "tree24": (24, 3, False, False, 15),
    "tree64": (64, 8, False, False, 16),
    "tree65": (65, 4, False, False, 17),
    "tree256": (256, 8, False, False, 43),
}


def make_case(name, B=1):
    """The inputs of a case for a batch of B problems on one tree: starting pose identity + N(0, 0.1^2), targets = the handles'
    positions under a second pose identity + N(0, 0.25^2) (reachable); with solve_translation the second pose is also shifted."""
    J, E, chain, trans, seed = CASES[name]
    joints, parents = tree(J, seed, chain)
    handles = deepest(parents, E)
    rng = np.random.default_rng(seed + 1000)
    q0 = np.stack([pose(J, 0.1, rng) for _ in range(B)])
    gt0 = rng.normal(0, 0.05, (B, 3)).astype(np.float32)
    targets = np.zeros((B, E, 3), np.float32)
    for b in range(B):
        gt1 = gt0[b] + (rng.normal(0, 0.1, 3).astype(np.float32) if trans else 0)
        targets[b] = fk(joints.astype(np.float64), parents, pose(J, 0.25, rng).astype(np.float64), gt1.astype(np.float64))[2][handles]
    return {"name": name, "joints": joints, "parents": parents, "handles": handles, "q0": q0, "gt0": gt0, "targets": targets,
            "solve_translation": trans, "extent": float(extent_of(joints)), "J": J, "E": E, "B": B}


def solve_case(case, iterations, dtype=np.float64, snapshots=None, **kw):
    """The oracle on every problem of a case: stacked (B, ...) arrays (with ``snapshots``: a dict of those per iteration count)."""
    outs = [solve(case["joints"], case["parents"], case["q0"][b], case["gt0"][b], kw.get("handles", case["handles"]),
                  kw.get("targets", case["targets"])[b], weights=kw.get("weights"), locked=kw.get("locked"), iterations=iterations,
                  damping=kw.get("damping"), max_step=kw.get("max_step"), solve_translation=case["solve_translation"], dtype=dtype,
                  snapshots=snapshots)
            for b in range(case["B"])]
    stack = lambda rs: {k: np.stack([o[k] for o in rs]) for k in rs[0]}  # noqa: E731
    return stack(outs) if snapshots is None else {n: stack([o[n] for o in outs]) for n in snapshots}
