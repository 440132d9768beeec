"""NumPy restatement of riggs_amd.arap (csrc/arap.hip): ARAP handle editing of control nodes.

float64 is the oracle; float32 (every operation rounded, the operator rounded to float32 as the kernel reads it, a float32 SVD) is
the yardstick for rounding.  The restatement fits rotations with an SVD and the Kabsch flip, as the reference does
(utils/arap_deform.py:136-146); the kernel uses Horn's quaternion form of the same problem.

  graph            cal_connectivity_from_points with adaptive weighting; the mean over the KEPT edges, weight 0 on a dropped edge
  laplacian        A = L_opt = I - W
  operator         G: rows of pinv(A_u) for the free nodes, zero rows for the handles; singular values <= rcond * largest dropped
  deform           x_init = rest positions with the handles moved; every solve x = x_init + G (b - A x_init)
"""
import functools
import json
import os

import numpy as np

LEAST_EDGE_NUM = 3


# ------------------------------------------------------------------------------------------------ the graph
def graph(points, radius, K, trajectory=None):
    """-> nn_idx (N, K) int32 with -1 = dropped, nn_dist (N, K) float32 with inf there, weight (N, K) float32.  float32 throughout,
    as the module builds it: the graph is an INPUT of the drag."""
    feat = np.asarray(points, np.float32) if trajectory is None else \
        (np.asarray(trajectory, np.float32).reshape(len(trajectory), -1) / np.float32(np.shape(trajectory)[1]))
    N = feat.shape[0]
    d = np.zeros((N, N), np.float32)
    for c in range(feat.shape[1]):
        diff = feat[:, None, c] - feat[None, :, c]
        d = d + diff * diff
    order = np.argsort(d, axis=1, kind="stable")[:, 1:K + 1]
    nn_dist = np.take_along_axis(d, order, 1)
    kept = np.ones((N, K), bool)
    kept[:, LEAST_EDGE_NUM:] = nn_dist[:, LEAST_EDGE_NUM:] < np.float32(radius) ** 2
    nn_idx = np.where(kept, order, -1).astype(np.int32)
    nn_dist = np.where(kept, nn_dist, np.float32(np.inf)).astype(np.float32)
    return nn_idx, nn_dist, weights_of(nn_dist)


def weights_of(nn_dist, dtype=np.float32):
    """exp(-d / mean over the kept edges), 0 on a dropped edge (d = inf), rows normalised: the reference's formula over the kept edges."""
    nn_dist = np.asarray(nn_dist, dtype)
    kept = np.isfinite(nn_dist)
    mean = (np.where(kept, nn_dist, 0).sum(dtype=dtype) / dtype(kept.sum())).astype(dtype)
    with np.errstate(invalid="ignore"):
        w = np.where(kept, np.exp(-np.where(kept, nn_dist, 0) / mean), 0).astype(dtype)
    return (w / w.sum(axis=1, keepdims=True)).astype(dtype)


def laplacian(nn_idx, weight):
    N, K = nn_idx.shape
    A = np.eye(N)
    for k in range(K):
        rows = np.nonzero(nn_idx[:, k] >= 0)[0]
        A[rows, nn_idx[rows, k]] = -np.asarray(weight, np.float64)[rows, k]
    return A


def operator(A, handles, rcond=1e-6):
    """-> (G (N, N) float64, null_dims)."""
    N = A.shape[0]
    free = np.ones(N, bool)
    free[list(handles)] = False
    U, s, Vt = np.linalg.svd(A[:, free], full_matrices=False)
    keep = s > rcond * s.max()
    inv = np.where(keep, 1.0 / np.where(keep, s, 1.0), 0.0)
    G = np.zeros((N, N))
    G[free] = (Vt.T * inv[None]) @ U.T
    return G, int((~keep).sum())


# ------------------------------------------------------------------------------------------------ the rotation fit
def fit_rotations(S):
    """Per 3x3 covariance S = sum src tgt^T the proper rotation maximising tr(R S): V U^T, and where det <= 0 the column of U of the
    smallest singular value flipped (arap_deform.py:136-146).  In S's dtype."""
    U, sig, Vt = np.linalg.svd(S)
    V = np.swapaxes(Vt, -1, -2)
    R = V @ np.swapaxes(U, -1, -2)
    flip = np.nonzero(np.linalg.det(R) <= 0)[0]
    if flip.size:
        Um = U.copy()
        Um[flip, :, np.argmin(sig[flip], axis=1)] *= -1
        R[flip] = V[flip] @ np.swapaxes(Um[flip], -1, -2)
    return R.astype(S.dtype)


def matrix_to_quaternion(R):
    """(w, x, y, z): the candidate of the largest of the four |component| estimates, no sign fix (utils/time_utils.py:146-205)."""
    dt = R.dtype
    m = R.reshape(-1, 9)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (m[:, i] for i in range(9))
    one = dt.type(1)
    a = np.stack([one + m00 + m11 + m22, one + m00 - m11 - m22, one - m00 + m11 - m22, one - m00 - m11 + m22], -1)
    qa = np.sqrt(np.maximum(a, 0)).astype(dt)
    cand = np.stack([np.stack([qa[:, 0] * qa[:, 0], m21 - m12, m02 - m20, m10 - m01], -1),
                     np.stack([m21 - m12, qa[:, 1] * qa[:, 1], m10 + m01, m02 + m20], -1),
                     np.stack([m02 - m20, m10 + m01, qa[:, 2] * qa[:, 2], m12 + m21], -1),
                     np.stack([m10 - m01, m20 + m02, m21 + m12, qa[:, 3] * qa[:, 3]], -1)], 1)
    pick = np.argmax(qa, axis=1)
    rows = np.arange(len(m))
    den = dt.type(2) * np.maximum(qa[rows, pick], dt.type(0.1))
    return (cand[rows, pick] / den[:, None]).astype(dt).reshape(R.shape[:-2] + (4,))


def rotation_angle(qa, qb):
    """The angle (rad) between the rotations of two quaternion arrays; q and -q are one rotation.  Well conditioned near 0: from the
    vector part of conj(qa) qb, not from acos of the dot product."""
    a, b = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    b = b / np.linalg.norm(b, axis=-1, keepdims=True)
    w = (a * b).sum(-1)
    v = a[..., :1] * b[..., 1:] - b[..., :1] * a[..., 1:] - np.cross(a[..., 1:], b[..., 1:])
    return 2.0 * np.arctan2(np.linalg.norm(v, axis=-1), np.abs(w))


# ------------------------------------------------------------------------------------------------ the drag
def deform(verts, nn_idx, weight, G, handles, handle_pos, init_verts=None, iterations=3, dtype=np.float64):
    """One drag -> (positions (N, 3), quaternions (N, 4), rotations (N, 3, 3)), all in ``dtype``."""
    dt = np.dtype(dtype).type
    p0 = np.asarray(verts, dtype)
    w = np.asarray(weight, dtype)
    G = np.asarray(G, dtype)
    N, K = nn_idx.shape
    kept = nn_idx >= 0
    j = np.where(kept, nn_idx, 0)
    xi = p0.copy()
    xi[list(handles)] = np.asarray(handle_pos, dtype)
    R = np.broadcast_to(np.eye(3, dtype=dtype), (N, 3, 3)).copy()
    if init_verts is None:
        d = p0 - xi
        r = d.copy()
        for k in range(K):
            r = r - np.where(kept[:, k, None], w[:, k, None] * d[j[:, k]], dt(0))
        x = xi + (G @ r).astype(dtype)
    else:
        x = np.asarray(init_verts, dtype).copy()
    P = np.where(kept[..., None], p0[:, None] - p0[j], dt(0))                       # (N, K, 3)
    for _ in range(iterations):
        Q = np.where(kept[..., None], x[:, None] - x[j], dt(0))
        S = np.zeros((N, 3, 3), dtype)
        for k in range(K):
            S = S + w[:, k, None, None] * (P[:, k, :, None] * Q[:, k, None, :])
        unchanged = (P == Q).all(axis=1).any(axis=-1)                                # (arap_deform.py:133-134)
        S[unchanged] = 0
        R = fit_rotations(S)
        R[unchanged | ~(np.abs(S).reshape(N, 9).max(1) > 0)] = np.eye(3, dtype=dtype)
        b = np.zeros((N, 3), dtype)
        ax = xi.copy()
        for k in range(K):
            v = np.einsum("nrc,nc->nr", (R + R[j[:, k]]).astype(dtype), P[:, k]).astype(dtype)
            b = b + np.where(kept[:, k, None], w[:, k, None] * v, dt(0))
            ax = ax - np.where(kept[:, k, None], w[:, k, None] * xi[j[:, k]], dt(0))
        r = dt(0.5) * b - ax
        x = xi + (G @ r).astype(dtype)
    return x.astype(dtype), matrix_to_quaternion(R), R


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
def cloud(kind, N, rng):
    if kind == "cube":
        return rng.uniform(-0.5, 0.5, (N, 3)).astype(np.float32)
    if kind == "blob":  # a Gaussian blob: under the editor's radius (extent / 8) the far columns of its sparse outer nodes are dropped
        return (0.3 * rng.standard_normal((N, 3))).astype(np.float32)
    raise ValueError(kind)


def extent_of(verts):
    return float(np.linalg.norm(np.asarray(verts, np.float64).max(0) - np.asarray(verts, np.float64).min(0)))


# name, N, M, B, K, cloud, radius (None = extent / 8, the editor's), iterations, init_verts given
CASES = [dict(name=n, N=N, M=M, B=B, K=K, kind=kind, radius=radius, iterations=it, init=init, seed=seed)
         for seed, (n, N, M, B, K, kind, radius, it, init) in enumerate([
             ("n17_m1_b1_k16", 17, 1, 1, 16, "cube", 10.0, 3, False),      # K = 16 at its smallest N; fewer nodes than a wave
             ("n65_m3_b3_k16", 65, 3, 3, 16, "cube", 10.0, 3, False),      # one node past a wave
             ("n300_m8_b1_k16_blob", 300, 8, 1, 16, "blob", None, 3, False),  # not a multiple of 64; dropped edges present
             ("n1024_m2_b2_k16", 1024, 2, 2, 16, "cube", None, 3, False),   # the limit
             ("n65_m3_b2_k4", 65, 3, 2, 4, "cube", 10.0, 3, False),
             ("n130_m2_b1_k10", 130, 2, 1, 10, "cube", 0.3, 3, False),
             ("n65_m3_b1_k16_it0", 65, 3, 1, 16, "cube", 10.0, 0, False),
             ("n65_m3_b1_k16_it1", 65, 3, 1, 16, "cube", 10.0, 1, False),
             ("n65_m3_b3_k16_init", 65, 3, 3, 16, "cube", 10.0, 3, True),
             ("n300_m8_b2_k10_blob_init_it1", 300, 8, 2, 10, "blob", None, 1, True),
         ], start=11)]


@functools.lru_cache(maxsize=None)
def _case_inputs(name):
    case = next(c for c in CASES if c["name"] == name)
    rng = np.random.default_rng(case["seed"])
    verts = cloud(case["kind"], case["N"], rng)
    ext = extent_of(verts)
    radius = ext / 8 if case["radius"] is None else case["radius"]
    handles = tuple(int(h) for h in rng.choice(case["N"], case["M"], replace=False))
    step = rng.uniform(0.1, 0.3, (case["B"], 1, 1)) * ext * _unit(rng.standard_normal((case["B"], 1, 3)))
    handle_pos = (verts[list(handles)][None] + step + 0.03 * ext * rng.standard_normal((case["B"], case["M"], 3))).astype(np.float32)
    init = (verts[None] + 0.03 * ext * rng.standard_normal((case["B"], case["N"], 3))).astype(np.float32) if case["init"] else None
    return dict(verts=verts, extent=ext, radius=np.float32(radius), handles=handles, handle_pos=handle_pos, init_verts=init)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def case_inputs(case):
    """The case's arrays: computed once, shared, never changed."""
    return _case_inputs(case["name"])


def reference(case, nn_idx, weight):
    """-> (o64, o32): ``pos`` (B, N, 3) and ``quat`` (B, N, 4) of the float64 oracle and of the float32 yardstick over the graph
    handed in (the graph is an input of the drag), and ``null_dims``."""
    inp = case_inputs(case)
    G, null_dims = operator(laplacian(nn_idx, weight), inp["handles"])
    out = []
    for dtype, op in ((np.float64, G), (np.float32, G.astype(np.float32))):
        res = [deform(inp["verts"], nn_idx, weight, op, inp["handles"], inp["handle_pos"][b],
                      None if inp["init_verts"] is None else inp["init_verts"][b], case["iterations"], dtype)
               for b in range(case["B"])]
        out.append(dict(pos=np.stack([r[0] for r in res]), quat=np.stack([r[1] for r in res]), null_dims=null_dims))
    return tuple(out)


_REF = {}


def case_reference(case, nn_idx, weight):
    """``reference`` over the module's own graph on the device: computed once per case, shared, never changed."""
    if case["name"] not in _REF:
        _REF[case["name"]] = reference(case, nn_idx, weight)
    return _REF[case["name"]]


def merge_report(env, section, records):
    """Behind a module's tests: ``records`` goes as JSON under ``section`` into the file the environment variable ``env`` names,
    next to what another module wrote there."""
    path = os.environ.get(env)
    if not (records and path):
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    whole = {}
    if os.path.exists(path):
        with open(path) as f:
            whole = json.load(f)
    whole[section] = records
    with open(path, "w") as f:
        json.dump(whole, f, indent=1, sort_keys=True)
