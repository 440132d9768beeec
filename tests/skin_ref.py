"""Float64 references of the skeleton deformation kernels (csrc/fk_device.h, csrc/deform.hip) with per-element bounds.

Each kernel is checked on its own, from the SAME fp32 inputs it read: the chain from (local_rot, joints, parents, the
cotangents), the skinning from the kernel's own transforms / node_rot.  A float64 evaluation of those inputs is exact to ~1e-15,
so what remains between kernel and reference is the kernel's fp32 arithmetic, bounded here per element.  Values and gradients
come from float64 autograd (no hand-derived gradient is shared with the kernels); closed forms appear only in the magnitudes
that scale the bounds.  u = 2^-24.

Chain (fk_forward_*, fk_backward_*).  T_j = [R(q_j) | c - R c] is off by E_T <= 20 u per rotation entry (two_s = 2/|q|^2 and
one product of two sums) and by the rounding of c - R c in its column.  Level by level G_j = G_p T_j gives
    E_j = 4 u |G_p||T_j| + E_p |T_j| + |G_p| E_T_j            (augmented 4x4 products, |.| elementwise),
so the bound grows with depth: a 256-joint chain has 255 levels.  The reverse sweep is bounded the same way: a parent's
dL/dG is its own term plus its children's A_c = dG_c T_c^T added one by one (nc + 1 terms), dT_j = R_p^T dG_j uses the
sweep's own G_p (off by E_p), and dq follows the kernel's closed form, whose magnitude (every product taken absolutely) scales
the rounding.

Top-K selection.  bone_d2 is written with contraction off (``#pragma clang fp contract(off)``, len2c staged with __f*_rn
operations), but deform.hip is compiled with -ffp-contract=fast, under which clang ignores that pragma, and __fmul_rn /
__fadd_rn are plain operations: on gfx950 the t numerator, a + t ba, the sum of squares and the staged len2c all become FMAs.
``bone_d2_f32`` restates the NON-contracted form in numpy float32 (what deform.hip:122-124 promises) and does not reproduce
the kernel's choice on every row.  The kernel's nn_idx is therefore checked by a float64 rule (``selection_violations``):
every selected bone's d2 <= every unselected bone's d2 + the d2 error bound below (which holds for the fused form too: an
FMA rounds once where a product and a sum round twice), in ascending order within that bound.

Skinning forward.  Per Gaussian and bone, x = d2 inv2r2 and w = exp(-x) (weight_mod) + 1e-7.  The relative error of w is
    rel = 10 u x                       (inv2r2 through expf and 1/(2 r^2), the product, x * LOG2E and LOG2E itself)
        + 16 u inv2r2 (|e|^2 + |t ba|^2)  (bone_d2(_fast): d2 is stationary in t, so only the rounding of e, t ba and the squares)
        + (2 EXP_ULP + 2) u            (v_exp_f32, stated as EXP_ULP ulp of its result, and the weight_mod product)
plus 2^-126 absolute (a result below the smallest normal may be flushed).  The sums over B bones add B u of their absolute
sums, and the normalisation and the final products a few u of the result.

Skinning backward.  Per bone, a sum over the N Gaussians: the bound is sum_n (|term error|) + L u sum_n |term|, with L the
depth of the kernel's reduction tree, derived from its structure (``depth_bonelane``, ``depth_topk``).  An any-order bound
(L = N) would be useless: at N = 300 000 it is 0.018 sum|t|, while a bone's gradient under random-sign cotangents is about
sum|t| / sqrt(N) = 0.002 sum|t|, so it would pass a zeroed bone.

Pure torch on whatever device the tensors live on; the skinning references work in slices of N so that the (N, B) float64
intermediates stay small.  tests/test_skin_ref_cpu.py shows on the host that these bounds reject the faults the GPU tests
(tests/test_gpu_wideskel_f64.py) are there to catch, and accept fp32 arithmetic summed in other orders.
"""
import numpy as np
import torch

from tests.mlp_ref import assert_within, violations  # noqa: F401  (re-exported: the same checker)

U = 2.0 ** -24
EXP_ULP = 2.0        # allowance for v_exp_f32, in ulp of its result (no accuracy figure is documented)
FLUSH = 2.0 ** -126  # a weight below the smallest normal may come out as 0
CX, CD, CE = 10.0, 16.0, 2.0 * EXP_ULP + 2.0


# ------------------------------------------------------------------------------------------------------------------ the chain
def quat_to_R(q):
    """quaternion_to_matrix with two_s = 2 / |q|^2 (un-normalised q), (J, 3, 3)."""
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    R = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def _parents(parents):
    vp = [int(p) for p in parents.tolist()]
    vp[0] = 0
    return vp


def local_T(q, joints, parents):
    """T_j = [R | c - R c] (J, 3, 4) about the PARENT joint c, and c."""
    vp = _parents(parents)
    c = joints[vp]
    R = quat_to_R(q)
    t = c - (R @ c[..., None])[..., 0]
    return torch.cat([R, t[..., None]], -1), c


def _aug(T):
    """(J, 3, 4) -> (J, 4, 4) with the row [0, 0, 0, 1]."""
    last = torch.zeros(T.shape[:-2] + (1, 4), dtype=T.dtype, device=T.device)
    last[..., 0, 3] = 1.0
    return torch.cat([T, last], -2)


def chain(q, joints, parents):
    """Global transforms G (J, 3, 4) and d_nodes without global_trans (J, 3) in the dtype of the inputs (autograd-able)."""
    T, _ = local_T(q, joints, parents)
    vp = _parents(parents)
    Ta = _aug(T)
    G = [T[0]]
    for j in range(1, T.shape[0]):
        G.append(G[vp[j]] @ Ta[j])
    G = torch.stack(G)
    posed = (G[:, :, :3] @ joints[..., None])[..., 0] + G[:, :, 3]
    return G, posed


def _local_T_err(q, c, R):
    aR = R.abs()
    ER = torch.full_like(R, 20 * U)
    Et = ER @ c.abs()[..., None]
    Et = Et[..., 0] + 4 * U * (aR @ c.abs()[..., None])[..., 0] + U * c.abs()
    return torch.cat([ER, Et[..., None]], -1)


def chain_forward(q, joints, parents, gt):
    """float64 references and bounds of riggs_fk_forward's transforms (J, 12) and d_nodes (J, 3)."""
    q64, j64, gt64 = q.double(), joints.double(), gt.double()
    T, c = local_T(q64, j64, parents)
    ET = _local_T_err(q64, c, T[:, :, :3])
    G, posed = chain(q64, j64, parents)
    vp = _parents(parents)
    aTa = _aug(T).abs()
    E = [ET[0]]
    for j in range(1, G.shape[0]):
        p = vp[j]
        aG, Ep = G[p].abs(), E[p]
        E.append(4 * U * (aG @ aTa[j]) + Ep @ aTa[j] + aG[:, :3] @ ET[j])
    E = torch.stack(E)
    xt = torch.cat([j64, torch.ones_like(j64[:, :1])], 1)
    dn = posed + gt64
    mag = (G.abs() @ xt.abs()[..., None])[..., 0]
    Edn = (E @ xt.abs()[..., None])[..., 0] + 5 * U * (mag + gt64.abs())
    return {"transforms": (G.reshape(-1, 12), E.reshape(-1, 12)), "d_nodes": (dn, Edn)}


def node_rot(transforms):
    """matrix_to_quaternion of the KERNEL's transforms (J, 12): float64 reference and bound.  The branch is the one the kernel
    takes: its four candidates a_c and their square roots are correctly rounded fp32 operations, restated in numpy."""
    m32 = transforms.detach().cpu().numpy().astype(np.float32).reshape(-1, 12)
    m00, m11, m22 = m32[:, 0], m32[:, 5], m32[:, 10]
    one = np.float32(1.0)
    a32 = np.stack([((one + m00) + m11) + m22, ((one + m00) - m11) - m22, ((one - m00) + m11) - m22, ((one - m00) - m11) + m22], 1)
    qa32 = np.where(a32 > 0, np.sqrt(np.maximum(a32, np.float32(0))), np.float32(0))
    pick = torch.from_numpy(np.argmax(qa32, 1)).to(transforms.device)
    m = transforms.double().reshape(-1, 12)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (m[:, i] for i in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    a = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], 1)
    cands = torch.stack([torch.stack([a[:, 0], m21 - m12, m02 - m20, m10 - m01], 1),
                         torch.stack([m21 - m12, a[:, 1], m10 + m01, m02 + m20], 1),
                         torch.stack([m02 - m20, m10 + m01, a[:, 2], m12 + m21], 1),
                         torch.stack([m10 - m01, m20 + m02, m21 + m12, a[:, 3]], 1)], 1)
    sel = torch.arange(m.shape[0], device=m.device)
    cand = cands[sel, pick]
    ap = a[sel, pick].clamp_min(0)
    qa = ap.sqrt()
    den = 2 * qa.clamp_min(0.1)
    ref = cand / den[:, None]
    Aabs = 1 + m00.abs() + m11.abs() + m22.abs()
    da = 3 * U * Aabs
    dqa = torch.where(qa > 0.1, da / (2 * qa.clamp_min(1e-30)) + U * qa, torch.zeros_like(qa))
    pair = torch.stack([(m21.abs() + m12.abs()), (m02.abs() + m20.abs()), (m10.abs() + m01.abs())], 1)
    pairs = torch.stack([torch.stack([a[:, 0] * 0, pair[:, 0], pair[:, 1], pair[:, 2]], 1),
                         torch.stack([pair[:, 0], a[:, 1] * 0, m10.abs() + m01.abs(), m02.abs() + m20.abs()], 1),
                         torch.stack([pair[:, 1], m10.abs() + m01.abs(), a[:, 2] * 0, m12.abs() + m21.abs()], 1),
                         torch.stack([pair[:, 2], m20.abs() + m02.abs(), m21.abs() + m12.abs(), a[:, 3] * 0], 1)], 1)
    dc = U * pairs[sel, pick]
    onehot = torch.nn.functional.one_hot(pick, 4).double()
    dc = dc + onehot * (da + 3 * U * ap)[:, None]
    bnd = dc / den[:, None] + cand.abs() * (2 * dqa / den ** 2)[:, None] + 2 * U * ref.abs()
    return ref, bnd


# the kernel's closed form of dL/dq from dR (fk_dq_from_dT): coefficient lists (factor, q index, dR index) of g_r, g_i, g_j, g_k
_GQ = ([(-1, 3, 1), (1, 2, 2), (1, 3, 3), (-1, 1, 5), (-1, 2, 6), (1, 1, 7)],
       [(1, 2, 1), (1, 3, 2), (1, 2, 3), (-2, 1, 4), (-1, 0, 5), (1, 3, 6), (1, 0, 7), (-2, 1, 8)],
       [(-2, 2, 0), (1, 1, 1), (1, 0, 2), (1, 1, 3), (1, 3, 5), (-1, 0, 6), (1, 3, 7), (-2, 2, 8)],
       [(-2, 3, 0), (-1, 0, 1), (1, 1, 2), (1, 0, 3), (-2, 3, 4), (1, 2, 5), (1, 1, 6), (1, 2, 7)])
# A = (R - I) / s: entries as lists of (factor, q index, q index)
_AQ = ([(-1, 2, 2), (-1, 3, 3)], [(1, 1, 2), (-1, 3, 0)], [(1, 1, 3), (1, 2, 0)],
       [(1, 1, 2), (1, 3, 0)], [(-1, 1, 1), (-1, 3, 3)], [(1, 2, 3), (-1, 1, 0)],
       [(1, 1, 3), (-1, 2, 0)], [(1, 2, 3), (1, 1, 0)], [(-1, 1, 1), (-1, 2, 2)])


def _dq_abs(q, X):
    """The kernel's dq = s g(q, dR) - s^2 q (A(q) . dR) with every product taken absolutely, applied to X >= 0 (J, 9)."""
    aq = q.abs()
    s = 2.0 / (q * q).sum(-1)
    g = torch.stack([sum(abs(f) * aq[:, a] * X[:, b] for f, a, b in terms) for terms in _GQ], 1)
    A = torch.stack([sum(abs(f) * aq[:, a] * aq[:, b] for f, a, b in e) for e in _AQ], 1)
    dotA = (A * X).sum(1)
    return s[:, None] * g + (s * s)[:, None] * aq * dotA[:, None]


def chain_backward(q, joints, parents, dG, gn):
    """float64 references and bounds of riggs_fk_backward's dL/dlocal_rot (J, 4) and dL/dglobal_trans (3) (added to zeros),
    for cotangents dG (J, 12) and gn (J, 3) (or None)."""
    J = q.shape[0]
    q64 = q.double().clone().requires_grad_(True)
    j64 = joints.double()
    dG64 = dG.double().reshape(J, 3, 4)
    gn64 = torch.zeros(J, 3, dtype=torch.float64, device=q.device) if gn is None else gn.double()
    G, posed = chain(q64, j64, parents)
    ((G * dG64).sum() + (posed * gn64).sum()).backward()
    dq_ref = q64.grad.detach()
    dgt_ref = gn64.sum(0)
    with torch.no_grad():
        fw = chain_forward(q, joints, parents, torch.zeros(3, device=q.device))
        E_G = fw["transforms"][1].reshape(J, 3, 4)
        Gd = G.detach()
        T, c = local_T(q.double(), j64, parents)
        ET = _local_T_err(q.double(), c, T[:, :, :3])
        aTa = _aug(T).abs()
        ETa = torch.cat([ET, torch.zeros_like(ET[:, :1])], 1)
        vp = _parents(parents)
        xt = torch.cat([j64, torch.ones_like(j64[:, :1])], 1)
        M = list(dG64.abs() + gn64.abs()[:, :, None] * xt.abs()[:, None, :])
        E = [2 * U * m for m in M]
        nkids = [0] * J
        for j in range(1, J):
            nkids[vp[j]] += 1
        for j in range(J - 1, 0, -1):  # children have larger indices: j is final here
            E[j] = E[j] + nkids[j] * U * M[j]
            p = vp[j]
            MA = M[j] @ aTa[j].t()
            M[p] = M[p] + MA
            E[p] = E[p] + E[j] @ aTa[j].t() + 4 * U * MA + M[j] @ ETa[j].t()
        E[0] = E[0] + nkids[0] * U * M[0]
        M, E = torch.stack(M), torch.stack(E)
        # dT_j = R_p^T dG_j (the root: dG_0), with the sweep's own G_p
        Rp = Gd[vp, :, :3].abs()
        ERp = E_G[vp, :, :3]
        MdT = Rp.transpose(1, 2) @ M
        EdT = Rp.transpose(1, 2) @ E + ERp.transpose(1, 2) @ M + 3 * U * MdT
        MdT[0], EdT[0] = M[0], E[0]
        ac = c.abs()
        MdR = MdT[:, :, :3] + MdT[:, :, 3:] * ac[:, None, :]
        EdR = EdT[:, :, :3] + EdT[:, :, 3:] * ac[:, None, :] + 2 * U * MdR
        qd = q.double()
        bq = _dq_abs(qd, EdR.reshape(J, 9)) + 16 * U * _dq_abs(qd, MdR.reshape(J, 9))
        bgt = J * U * gn64.abs().sum(0)
    return {"dL/dlocal_rot": (dq_ref, bq), "dL/dglobal_trans": (dgt_ref, bgt)}


# ------------------------------------------------------------------------------------------------------- the top-K selection
def bone_d2_f32(x, joints, parents):
    """bone_d2 (deform.hip) in numpy float32 as written, without contraction: (N, B) float32."""
    x = np.asarray(x, np.float32)
    jt = np.asarray(joints, np.float32)
    par = np.asarray(parents, np.int64)
    a = jt[par[1:]]
    ba = (jt[1:] - a).astype(np.float32)
    l2 = (ba[:, 0] * ba[:, 0] + ba[:, 1] * ba[:, 1]) + ba[:, 2] * ba[:, 2]
    len2c = np.maximum(l2, np.float32(1e-6)).astype(np.float32)
    px, py, pz = x[:, 0:1], x[:, 1:2], x[:, 2:3]
    ex, ey, ez = px - a[None, :, 0], py - a[None, :, 1], pz - a[None, :, 2]
    t = ((ex * ba[None, :, 0] + ey * ba[None, :, 1]) + ez * ba[None, :, 2]) / len2c[None]
    t = np.minimum(np.maximum(t, np.float32(0)), np.float32(1))
    sx = (a[None, :, 0] + t * ba[None, :, 0]) - px
    sy = (a[None, :, 1] + t * ba[None, :, 1]) - py
    sz = (a[None, :, 2] + t * ba[None, :, 2]) - pz
    d2 = (sx * sx + sy * sy) + sz * sz
    assert d2.dtype == np.float32
    return d2


def topk_select(x, joints, parents, K):
    """The selection of the non-contracted bone_d2: (N, K) int64 bone indices (0-based: joint index - 1) in ascending (d2, index)
    order.  (The kernel's contracted arithmetic may differ on near-tied rows: see the module docstring.)"""
    d2 = bone_d2_f32(x, joints, parents)
    return np.argsort(d2, axis=1, kind="stable")[:, :K]


# ---------------------------------------------------------------------------------------------------------- the skinning
def _geom(x, a, ba, l2):
    e = x[:, None, :] - a[None]
    t = ((e * ba[None]).sum(-1) / l2.clamp_min(1e-6)[None]).clamp(0.0, 1.0)
    s = t[..., None] * ba[None] - e
    d2 = (s * s).sum(-1)
    de2 = (e * e).sum(-1) + t * t * l2[None]
    return d2, de2


def _bones(joints, parents, rho, transforms, nrot):
    j64 = joints.double()
    par = parents.long()
    a = j64[par[1:]]
    ba = j64[1:] - a
    return a, ba, (ba * ba).sum(-1), rho.double()[1:], transforms.double().reshape(-1, 12)[1:], nrot.double()[1:]


def depth_bonelane(N, J, gpb=1024):
    """Depth of the bone-lane backward's reduction tree over the Gaussians (per-bone sums; dL/dglobal_trans the same): a lane
    adds its slot's gpb/32 Gaussians in sequence, 3 xor levels fold the 8 slots, 4 waves add into LDS, and the finish kernel
    adds ceil(parts / 256) partials per thread, 6 levels of wave_sum and a 2-level 4-way sum."""
    parts = max(1, -(-N // gpb))
    return gpb // 32 + 3 + 4 + -(-parts // 256) + 6 + 2 + 6  # (+6: the lane's gt/step adds and the partial's store round trip)


def depth_topk(N):
    """Depth of the top-K backward's reduction: 6-level wave_sum, 4 waves of LDS atomics, one global atomic per workgroup
    (ceil(N / 256) of them, in any order)."""
    return 6 + 4 + -(-N // 256) + 2


def skin(x, joints, parents, rho, transforms, nrot, gt, mask=None, wm=None, sel=None, cot=None, depth=None, chunk=16384):
    """float64 references and bounds of riggs_lbs_forward (d_xyz, d_rotation, nn_weight) and, with ``cot`` = (g_xyz, g_rot),
    of riggs_lbs_backward (dL/dtransforms, dL/dnode_radius_log, dL/dglobal_trans, dL/dmotion_mask, dL/dweight_mod).
    ``transforms`` / ``nrot``: the kernel's own (J, 12) / (J, 4); ``sel``: (N, K) bone indices (the selection, in its order) or
    None for all bones; ``depth``: the reduction depth L of the backward kernel over N.  Each entry is (ref, bound)."""
    dev = x.device
    N, J = x.shape[0], joints.shape[0]
    B = J - 1
    a, ba, l2, rho_b, Gb, qb = _bones(joints, parents, rho, transforms, nrot)
    nB = B if sel is None else sel.shape[1]
    gt64 = gt.double()
    out = {k: [] for k in ("d_xyz", "d_rotation", "nn_weight", "dmask", "dmod")}
    bnd = {k: [] for k in out}
    back = cot is not None
    if back:
        Gp = Gb.clone().requires_grad_(True)
        rp = rho_b.clone().requires_grad_(True)
        gtp = gt64.clone().requires_grad_(True)
        aG = Gb.abs()
        acc_bG = torch.zeros(B, 12, dtype=torch.float64, device=dev)
        acc_br = torch.zeros(B, dtype=torch.float64, device=dev)
        L = depth
    else:
        Gp, rp, gtp = Gb, rho_b, gt64
    ggt_sum = torch.zeros(3, dtype=torch.float64, device=dev)
    for s in range(0, max(N, 1), chunk):
        e_ = min(N, s + chunk)
        if e_ <= s:
            break
        xs = x[s:e_].double()
        n = xs.shape[0]
        ms = torch.ones(n, dtype=torch.float64, device=dev) if mask is None else mask.reshape(-1)[s:e_].double()
        ws = None if wm is None else wm[s:e_].double()
        if sel is None:
            selm = torch.ones(n, B, dtype=torch.float64, device=dev)
        else:
            selm = torch.zeros(n, B, dtype=torch.float64, device=dev)
            selm.scatter_(1, sel[s:e_].to(dev).long(), 1.0)
        with torch.no_grad():
            d2, de2 = _geom(xs, a, ba, l2)
        if back:
            ms = ms.clone().requires_grad_(True)
            if ws is not None:
                ws = ws.clone().requires_grad_(True)
        inv2r2 = 0.5 * torch.exp(-2.0 * rp)
        xk = d2 * inv2r2[None]
        ek = torch.exp(-xk)
        wr = ek if ws is None else ek * ws
        v = (wr + 1e-7) * selm
        S = v.sum(1)
        xt = torch.cat([xs, torch.ones_like(xs[:, :1])], 1)
        Mm = (v @ Gp).reshape(n, 3, 4)
        num = (Mm @ xt[..., None])[..., 0]
        ax0 = num / S[:, None]
        dxyz = (ax0 + gtp[None] - xs) * ms[:, None]
        Q = v @ qb
        drot = Q / S[:, None] * ms[:, None]
        with torch.no_grad():
            vd, Sd, xkd, ekd, wrd = v.detach(), S.detach(), xk.detach(), ek.detach(), wr.detach()
            i2 = inv2r2.detach()
            rel = CX * U * xkd + CD * U * i2[None] * de2 + CE * U
            dv = (wrd * rel + FLUSH + U * (wrd + 1e-7)) * selm
            dS = dv.sum(1) + nB * U * Sd
            axt = xt.abs()
            y = dv + (nB + 4) * U * vd
            dnum = ((y @ Gb.abs()).reshape(n, 3, 4) @ axt[..., None])[..., 0]
            anum = num.detach().abs()
            dax = dnum / Sd[:, None] + anum * dS[:, None] / Sd[:, None] ** 2 + 2 * U * anum / Sd[:, None]
            am = ms.detach().abs()[:, None]
            a0, agt = ax0.detach().abs(), gt64.abs()[None]
            b_dxyz = am * (dax + U * (a0 + agt) + U * ((ax0.detach() + gt64[None]).abs() + xs.abs())) + U * dxyz.detach().abs()
            dQ = (dv + nB * U * vd) @ qb.abs()
            aQ = Q.detach().abs()
            b_drot = am * (dQ / Sd[:, None] + aQ * dS[:, None] / Sd[:, None] ** 2 + 2 * U * aQ / Sd[:, None]) + U * drot.detach().abs()
            w = vd / Sd[:, None]
            dw = dv / Sd[:, None] + vd * (dS / Sd ** 2)[:, None] + 2 * U * w
            out["d_xyz"].append(dxyz.detach())
            bnd["d_xyz"].append(b_dxyz)
            out["d_rotation"].append(drot.detach())
            bnd["d_rotation"].append(b_drot)
            if sel is None:
                out["nn_weight"].append(w)
                bnd["nn_weight"].append(dw)
            else:
                ix = sel[s:e_].to(dev).long()
                out["nn_weight"].append(torch.gather(w, 1, ix))
                bnd["nn_weight"].append(torch.gather(dw, 1, ix))
        if not back:
            continue
        gx, gr = cot[0][s:e_].double(), cot[1][s:e_].double()
        loss = (dxyz * gx).sum() + (drot * gr).sum()
        inputs = [Gp, rp, ms] + ([ws] if ws is not None else [])
        grads = torch.autograd.grad(loss, inputs)
        with torch.no_grad():
            acc_bG += grads[0]
            acc_br += grads[1]
            ggt_sum += (gx * ms.detach()[:, None]).sum(0)
            out["dmask"].append(grads[2])
            if ws is not None:
                out["dmod"].append(grads[3])
            msd = ms.detach()
            gh, hh = gx * msd[:, None], gr * msd[:, None]
            agh, ahh, agx, agr = gh.abs(), hh.abs(), gx.abs(), gr.abs()
            # H[n, k, r] = sum_c |G_k[r, c]| |xt_n[c]|
            H = torch.einsum("krc,nc->nkr", aG.reshape(B, 3, 4), axt)
            Dw = (H * agh[:, None, :]).sum(-1) + ahh @ qb.abs().t()
            Du = (H * agx[:, None, :]).sum(-1) + agr @ qb.abs().t()
            Gv = (Gb.reshape(B, 3, 4)[None] @ xt[:, None, :, None])[..., 0]  # (n, B, 3): G_k xt
            dwv = (Gv * gh[:, None, :]).sum(-1) + hh @ qb.t()
            Sx = (w * dwv).sum(1)
            dSx = ((dw + (nB + 16) * U * w) * Dw).sum(1)
            dl = (dwv - Sx[:, None]) / Sd[:, None]
            ddl = (12 * U * Dw + dSx[:, None] + U * (dwv.abs() + Sx.abs()[:, None])) / Sd[:, None] \
                + (dwv - Sx[:, None]).abs() / Sd[:, None] * (dS / Sd + 2 * U)[:, None]
            weff = wrd * selm
            dxk = 8 * U * xkd + CD * U * i2[None] * de2
            r = 2 * dl * weff * xkd
            dr = 2 * (ddl * weff * xkd + dl.abs() * ((weff * rel + FLUSH * selm) * xkd + weff * dxk) + 5 * U * dl.abs() * weff * xkd)
            P = (agh[:, :, None] * axt[:, None, :]).reshape(n, 12)
            bG_part = (dw + (L + 3) * U * w).t() @ P
            br_part = (dr + (L + 2) * U * r.abs()).sum(0)
            if s == 0:
                bG_acc, br_acc, bgt_acc = bG_part, br_part, (L + 2) * U * agh.sum(0)
            else:
                bG_acc, br_acc, bgt_acc = bG_acc + bG_part, br_acc + br_part, bgt_acc + (L + 2) * U * agh.sum(0)
            bnd["dmask"].append((dw * Du).sum(1) + (nB + 16) * U * (w * Du).sum(1)
                                + 4 * U * (agx * (gt64.abs()[None] + xs.abs())).sum(1))
            if ws is not None:
                bnd["dmod"].append(ddl * ekd + dl.abs() * (ekd * (rel + U) + FLUSH))
    res = {}
    for k in ("d_xyz", "d_rotation", "nn_weight"):
        w_ = nB if k == "nn_weight" else (3 if k == "d_xyz" else 4)
        res[k] = (torch.cat(out[k]) if out[k] else torch.zeros(0, w_, dtype=torch.float64, device=dev),
                  torch.cat(bnd[k]) if bnd[k] else torch.zeros(0, w_, dtype=torch.float64, device=dev))
    if back:
        zG = torch.zeros(1, 12, dtype=torch.float64, device=dev)
        z1 = torch.zeros(1, dtype=torch.float64, device=dev)
        if N == 0:
            bG_acc = torch.zeros(B, 12, dtype=torch.float64, device=dev)
            br_acc = torch.zeros(B, dtype=torch.float64, device=dev)
            bgt_acc = torch.zeros(3, dtype=torch.float64, device=dev)
        res["dL/dtransforms"] = (torch.cat([zG, acc_bG]), torch.cat([zG, bG_acc]))
        res["dL/dnode_radius_log"] = (torch.cat([z1, acc_br]), torch.cat([z1, br_acc]))
        res["dL/dglobal_trans"] = (ggt_sum, bgt_acc)
        res["dL/dmotion_mask"] = (torch.cat(out["dmask"]) if out["dmask"] else torch.zeros(0, dtype=torch.float64, device=dev),
                                  torch.cat(bnd["dmask"]) if bnd["dmask"] else torch.zeros(0, dtype=torch.float64, device=dev))
        if wm is not None:
            res["dL/dweight_mod"] = (torch.cat(out["dmod"]) if out["dmod"] else torch.zeros(0, B, dtype=torch.float64, device=dev),
                                     torch.cat(bnd["dmod"]) if bnd["dmod"] else torch.zeros(0, B, dtype=torch.float64, device=dev))
    return res


def deform64(x, joints, parents, rho, q, gt, mask, sel=None):
    """deform_by_pose (chain and skinning) in float64 over a GIVEN selection ``sel`` (N, K) (None: all bones): d_xyz, d_rotation,
    d_nodes, autograd-able through q, gt, rho and mask.  For comparing gradients on rows where top-K distances tie: the kernel's
    selection is pinned exactly by ``topk_select``, and this is the deformation over it."""
    from oracle.deform_ref import matrix_to_quaternion
    x, joints = x.double(), joints.double()
    N, J = x.shape[0], joints.shape[0]
    G, posed = chain(q, joints, parents)
    nrot = matrix_to_quaternion(G[:, :, :3].detach())
    a, ba, l2, _, _, _ = _bones(joints, parents, rho.detach(), G.detach().reshape(J, 12), nrot)
    d2, _ = _geom(x, a, ba, l2)
    v = torch.exp(-d2 * (0.5 * torch.exp(-2.0 * rho[1:]))[None]) + 1e-7
    if sel is not None:
        selm = torch.zeros(N, J - 1, dtype=torch.float64, device=x.device)
        selm.scatter_(1, sel.to(x.device).long(), 1.0)
        v = v * selm
    S = v.sum(1)
    xt = torch.cat([x, torch.ones_like(x[:, :1])], 1)
    ax = ((v @ G[1:].reshape(J - 1, 12)).reshape(N, 3, 4) @ xt[..., None])[..., 0] / S[:, None] + gt[None]
    m = mask.reshape(N, 1)
    return {"d_xyz": (ax - x) * m, "d_rotation": (v @ nrot[1:]) / S[:, None] * m, "d_nodes": posed + gt[None]}


def selection_violations(x, joints, parents, sel):
    """Rows where the selection ``sel`` (N, K) (0-based bones, in the kernel's order) breaks the float64 rule: every selected bone's
    d2 <= every unselected bone's d2 + the d2 error bound, and the selected bones in ascending d2 within that bound."""
    x64 = torch.as_tensor(x).double()
    j64 = torch.as_tensor(joints).double()
    par = torch.as_tensor(parents).long()
    a = j64[par[1:]]
    ba = j64[1:] - a
    d2, de2 = _geom(x64, a, ba, (ba * ba).sum(-1))
    bd = CD * U * de2
    sel = torch.as_tensor(sel).long()
    N, B = d2.shape
    if sel.shape[1] == 0 or N == 0:
        return 0
    taken = torch.zeros(N, B, dtype=torch.bool).scatter_(1, sel, True)
    lo, hi = d2 - bd, d2 + bd
    worst_sel = torch.where(taken, lo, torch.full_like(lo, -float("inf"))).amax(1)
    best_free = torch.where(taken, torch.full_like(hi, float("inf")), hi).amin(1)
    bad = worst_sel > best_free
    ls, hs = torch.gather(lo, 1, sel), torch.gather(hi, 1, sel)
    if sel.shape[1] > 1:
        bad |= (ls[:, :-1] > hs[:, 1:]).any(1)
    return int(bad.sum())
