"""Float64 reference of the control-node blend (csrc/cnode.hip: riggs_cnode_forward / riggs_cnode_backward) with per-element bounds.

The kernels are checked from the SAME fp32 inputs they read and from the forward kernel's OWN neighbour lists ``nn_idx``: on given
lists the operation is smooth, a float64 evaluation is exact to ~1e-15, and what remains between kernel and reference is the
kernel's fp32 arithmetic, bounded here per element.  Values are the forward formulas of oracle/cnode_ref.py's docstring
(cal_nn_weight and forward, node_trans_bias = None) in float64 torch; every gradient is float64 AUTOGRAD of those formulas — no
hand-derived gradient is shared with the kernel.  Closed forms appear only in the magnitudes that scale the bounds.
oracle/cnode_ref.backward (hand-derived, numpy) is a second opinion: tests/test_cnode_ref_cpu.py holds the two to 1e-10.
u = 2^-24; EXP_ULP and FLUSH as in tests/skin_ref.py (an exponential is EXP_ULP ulp = 2 EXP_ULP u of its result, and a result
below the smallest normal may come out as 0); TINY = 2^-140 per product covers a product of normals that lands in the denormals.

Distance.  d = sum of D = 3 + hyper squares in one FMA chain (the zero padding of the float4 table adds exact zeros): every
difference is off by u, its square by 2 u, and the chain rounds D times: (D + 2) u d.  All terms are non-negative, so the bound
is relative.  The weights use DIST_W = (D + 2) u; the selection rule and nn_dist use DIST = 2 DIST_W (a comparison of two
distances carries both errors' second-order terms).

Weight.  r = expf(rho), r2 = r r: (4 EXP_ULP + 1) u.  t = d / (2 r2): DIST_W + (4 EXP_ULP + 1) u + u (the division; 2 r2 is
exact), and 2 u more for expf's own argument scaling.  e = expf(-t): rel_e = (DIST_W + (4 EXP_ULP + 4) u) t + 2 EXP_ULP u, plus
FLUSH absolute.  sigmoid = 1 / (1 + expf(-l)): (2 EXP_ULP + 2) u.  u_k = e sigmoid: rel_e + rel_sig + u.  v_k = u_k + 1e-7f: the
constant is rounded and the sum rounds: 2 u v_k.  S = sum_k v_k in sequence: sum dv + K u S.  w_k = v_k / S:
dw = dv / S + v dS / S^2 + u w.

Blend.  R(q) of q = local_rotation + (1, 0, 0, 0) is off by E_R = 24 u per entry (two_s = 2 / |q|^2 and one product of two sums,
20 u as in skin_ref, and the rounded q_0 = 1 + .).  y = R (x - n) + n + trans: dy = E_R |x - n|_1 + 6 u Ay, with Ay the sum of
the absolute terms.  sum_k w_k y_k: sum (dw Ay + w dy) + (K + 1) u sum w Ay; the subtraction of x, the mask product and the
rotation's bias each add u of their operands.

Per-Gaussian backward.  a_k ("dw" in the kernel) = m (g . y + h . rot + s . scale), ten products: da = m |g| . dy + 14 u A_k, A_k
the same sum with every product taken absolutely.  dv_k = (a_k - sum w a) / S: the subtraction cancels, so its error is scaled
by |a_k| + sum_j w_j |a_j| (through A), not by |dv_k|:
    d(dv_k) = (da_k + d(sum w a) + u (|a_k| + |sum w a|)) / S + |dv_k| (dS / S + 2 u),
    d(sum w a) = sum_j (dw_j A_j + w_j da_j) + (K + 1) u sum_j w_j A_j.
Each accumulator entry is a short product of dv_k, u_k or e_k, d_k, 1 / r2 and a coordinate difference; its error is the sum of
the factors' errors times the other factors (see ``blend``).  dL/dfeature sums K entries (K u of their absolute sum),
dL/dmotion_mask is a ten-term dot of the blend sums.

Node sums.  A node's gradient is the sum of its c entries' rows:  bound = sum(term error) + L u sum |term|, with L the depth
the reduce kernel's STRUCTURE gives: 32 row lanes take every 32nd row, each lane keeps four partial sums (rows 128 apart; up to
3 remainder rows go to the first), adds them as a 2-level tree, and lane 0..31 of the first wave sums the 32 lanes' results in
sequence: L = ceil(c / 128) + 2 + 2 + 31 = ceil(c / 128) + 35.  The rows of a segment are placed by an LDS atomicAdd, so their
order changes from run to run: the bound uses only the structure (which rows meet in a partial sum is free, how many do is not)
and holds for ANY placement.  L = c would be useless (see skin_ref's docstring): at c = 5000 it is 3e-4 sum|t| where a node's
gradient under random-sign cotangents is ~ sum|t| / 70.  The node-level chain rules (sigmoid', quaternion -> matrix) add their
own rounding: the kernel's closed form dq = s g(q, G) - s^2 q (A(q) . G) with every product taken absolutely (skin_ref._dq_abs),
applied to the bound of G and, times 16 u, to |G|.

An element whose bound is 0 is compared exactly (zero cotangent, mask 0, a node without entries): never vacuous.

Neighbour lists (``selection_violations``).  The forward keeps a sorted K-list with strict comparisons (ties keep the lower node
index).  Its fp32 distance is within DIST of the float64 one, so per Gaussian: K distinct indices in [0, M); entry k's float64
distance, lowered by DIST, does not exceed the k-th smallest float64 distance raised by DIST (the k nodes of smallest true
distance all have fp32 distance below that); ascending within DIST; where two nodes' coordinates are bit-identical their fp32
distances are equal, so the lower index comes first and is never left out in favour of the higher; nn_dist within DIST.

Pure torch on whatever device the tensors live on.
"""
import torch

from tests.mlp_ref import assert_within, violations  # noqa: F401  (re-exported: the same checker)
from tests.skin_ref import EXP_ULP, FLUSH, U, _dq_abs, quat_to_R

TINY = 2.0 ** -140
E_R = 24.0 * U
R2_REL = (4.0 * EXP_ULP + 1.0) * U
SIG_REL = (2.0 * EXP_ULP + 2.0) * U

NODE_KEYS = ("g_trans", "g_rot", "g_scale", "g_local_rot", "g_radius", "g_weight", "g_nodes_hyper")
GAUSS_KEYS = ("g_feature", "g_mask")
FWD_KEYS = ("d_xyz", "d_rotation", "d_scaling", "nn_weight", "nn_dist")


def dist_rel(hyper):
    return (3 + hyper + 2) * 2.0 * U


def depth_reduce(count):
    """Depth of cnode_node_reduce_kernel's sum over a node's ``count`` rows (tensor or int): see the module docstring."""
    return (count + 127) // 128 + 35


def _coords(x, feature, nodes, hyper):
    xa, na = x.double(), nodes[:, :3].double()
    if hyper:
        xa = torch.cat([xa, feature[:, :hyper].double()], 1)
        na = torch.cat([na, nodes[:, 3:3 + hyper].double()], 1)
    return xa, na


def true_lists(x, feature, nodes, hyper, K, chunk=4096):
    """The stable float64 argsort's lists (N, K) int64: ascending distance, ties to the lower index."""
    xa, na = _coords(x, feature, nodes, hyper)
    out = []
    for s in range(0, xa.shape[0], chunk):
        d = ((xa[s:s + chunk, None] - na[None]) ** 2).sum(-1)
        out.append(torch.sort(d, dim=1, stable=True).indices[:, :K])
    return torch.cat(out) if out else torch.zeros(0, K, dtype=torch.long, device=x.device)


def selection_violations(x, feature, nodes, hyper, nn_idx, nn_dist=None, chunk=4096):
    """Number of Gaussians whose list ``nn_idx`` (N, K) (and ``nn_dist``) breaks the float64 rule of the module docstring."""
    N, K = nn_idx.shape
    M = nodes.shape[0]
    if N == 0:
        return 0
    B = dist_rel(hyper)
    xa, na = _coords(x, feature, nodes, hyper)
    idx = nn_idx.long()
    bad = ((idx < 0) | (idx >= M)).any(1)
    idc = idx.clamp(0, M - 1)
    srt = torch.sort(idc, dim=1).values
    if K > 1:
        bad |= (srt[:, 1:] == srt[:, :-1]).any(1)
    # bit-identical nodes: (lo, hi) index pairs
    c32 = nodes[:, :3 + hyper].float().contiguous()
    _, inv = torch.unique(c32.view(torch.int32), dim=0, return_inverse=True)
    pairs = []
    order = torch.argsort(inv, stable=True).tolist()
    invl = inv.tolist()
    for a, b in zip(order[:-1], order[1:]):
        if invl[a] == invl[b]:
            grp = [j for j in order if invl[j] == invl[a]]
            pairs += [(p, q) for i, p in enumerate(grp) for q in grp[i + 1:] if (p, q) not in pairs]
    for lo, hi in pairs:
        has_lo, has_hi = (idc == lo), (idc == hi)
        pos_lo = torch.where(has_lo.any(1), has_lo.float().argmax(1), torch.full((N,), K, device=idc.device))
        pos_hi = torch.where(has_hi.any(1), has_hi.float().argmax(1), torch.full((N,), K, device=idc.device))
        bad |= has_hi.any(1) & (pos_lo > pos_hi)  # (lo missing: pos_lo = K)
    for s in range(0, N, chunk):
        e_ = min(N, s + chunk)
        d = ((xa[s:e_, None] - na[None]) ** 2).sum(-1)
        kth = torch.sort(d, dim=1).values[:, :K]
        sel = torch.gather(d, 1, idc[s:e_])
        b = sel * (1 - B) > kth * (1 + B)
        if K > 1:
            b[:, :-1] |= sel[:, :-1] * (1 - B) > sel[:, 1:] * (1 + B)
        if nn_dist is not None:
            nd = nn_dist[s:e_].double()
            b |= ~((nd - sel).abs() <= B * sel + TINY)
        bad[s:e_] |= b.any(1)
    return int(bad.sum())


def _scat(M, flat, vals):
    """Per-node sums of per-entry values (N, K, ...) -> (M, ...)."""
    tail = vals.shape[2:]
    out = torch.zeros((M,) + tuple(tail), dtype=torch.float64, device=vals.device)
    return out.index_add_(0, flat, vals.reshape((-1,) + tuple(tail)))


def blend(x, feature, mask, nodes, radius_log, weight_logit, attrs, nn_idx, hyper, local_frame, d_rot_as_res, cot=None):
    """float64 references and bounds of riggs_cnode_forward (FWD_KEYS) and, with ``cot`` = {"g_xyz", "g_rot", "g_scale"} (each a
    tensor or None for a NULL cotangent), of every gradient riggs_cnode_backward writes (NODE_KEYS, GAUSS_KEYS), on the lists
    ``nn_idx`` (N, K).  ``nodes``: (M, >= 3 + hyper), ``feature``: (N, >= hyper) or None, ``mask``: (N) or None, ``weight_logit``:
    (M) or None, ``attrs``: d_xyz, d_rotation, d_scaling and (local_frame) local_rotation.  Each entry is (ref, bound)."""
    dev = x.device
    N, M, K, D = x.shape[0], nodes.shape[0], nn_idx.shape[1], 3 + hyper
    idx = nn_idx.long()
    flat = idx.reshape(-1)
    f64 = dict(dtype=torch.float64, device=dev)
    E = torch.tensor([1.0, 0.0, 0.0, 0.0], **f64)
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)  # noqa: E731
    x64, n3 = x.double(), nodes[:, :3].double()
    fh = leaf(feature[:, :hyper]) if hyper else None
    nh = leaf(nodes[:, 3:D]) if hyper else None
    rho = leaf(radius_log.reshape(-1))
    wl = leaf(weight_logit.reshape(-1)) if weight_logit is not None else None
    tr, ro, sc = leaf(attrs["d_xyz"]), leaf(attrs["d_rotation"]), leaf(attrs["d_scaling"])
    lq = leaf(attrs["local_rotation"]) if local_frame else None
    m = leaf(mask.reshape(-1)) if mask is not None else None
    rel = x64[:, None] - n3[idx]
    d = (rel * rel).sum(-1)
    if hyper:
        diff = fh[:, None] - nh[idx]
        d = d + (diff * diff).sum(-1)
    r2 = torch.exp(2.0 * rho)[idx]
    t = d / (2.0 * r2)
    e = torch.exp(-t)
    u = e * torch.sigmoid(wl)[idx] if wl is not None else e
    v = u + 1e-7
    S = v.sum(1, keepdim=True)
    w = v / S
    if local_frame:
        R = quat_to_R(lq + E)
        y = (R[idx] @ rel[..., None])[..., 0] + n3[idx] + tr[idx]
    else:
        y = tr[idx]
    bias = 0.0 if d_rot_as_res else 1.0
    roe = ro + bias * E
    ts = (w[..., None] * y).sum(1) - (x64 if local_frame else 0.0)
    rs = (w[..., None] * roe[idx]).sum(1) - bias * E
    ss = (w[..., None] * sc[idx]).sum(1)
    mm = m[:, None] if m is not None else torch.ones(N, 1, **f64)
    dxyz, drot, dsc = ts * mm, rs * mm + bias * E, ss * mm
    res = {}
    with torch.no_grad():
        DIST, DIST_W = dist_rel(hyper), 0.5 * dist_rel(hyper)
        dd_, td, ed, ud, vd, Sd, wd, r2d = (q.detach() for q in (d, t, e, u, v, S, w, r2))
        rel_e = (DIST_W + R2_REL + 3 * U) * td + 2 * EXP_ULP * U
        de = ed * rel_e + FLUSH
        du = ud * (rel_e + (SIG_REL if wl is not None else 0.0) + U) + FLUSH
        dv = du + 2 * U * vd
        dS = dv.sum(1, keepdim=True) + K * U * Sd
        dw = dv / Sd + vd * dS / Sd ** 2 + U * wd
        arel = rel.abs()
        if local_frame:
            Ay = (R.detach().abs()[idx] @ arel[..., None])[..., 0] + n3[idx].abs() + tr.detach()[idx].abs()
            dy = E_R * arel.sum(-1, keepdim=True) + 6 * U * Ay
        else:
            Ay = tr.detach()[idx].abs()
            dy = torch.zeros_like(Ay)
        Aro, Asc = roe.detach()[idx].abs(), sc.detach()[idx].abs()
        dro = bias * U * Aro
        wAy, wAro, wAsc = ((wd[..., None] * A).sum(1) for A in (Ay, Aro, Asc))
        dts = (dw[..., None] * Ay + wd[..., None] * dy).sum(1) + (K + 1) * U * wAy
        if local_frame:
            dts = dts + U * (wAy + x64.abs())
        drs = (dw[..., None] * Aro + wd[..., None] * dro).sum(1) + (K + 1) * U * wAro + bias * U * (wAro + 1.0)
        dss = (dw[..., None] * Asc).sum(1) + (K + 1) * U * wAsc
        am = mm.detach().abs()
        res["d_xyz"] = (dxyz.detach(), am * dts + 2 * U * dxyz.detach().abs())
        res["d_rotation"] = (drot.detach(), am * drs + 2 * U * drot.detach().abs() + bias * U * E)
        res["d_scaling"] = (dsc.detach(), am * dss + 2 * U * dsc.detach().abs())
        res["nn_weight"] = (wd, dw)
        res["nn_dist"] = (dd_, DIST * dd_ + TINY * (dd_ > 0))
    if cot is None:
        return res
    z = lambda wdt: torch.zeros(N, wdt, **f64)  # noqa: E731
    g = z(3) if cot.get("g_xyz") is None else cot["g_xyz"].double()
    h = z(4) if cot.get("g_rot") is None else cot["g_rot"].double()
    s = z(3) if cot.get("g_scale") is None else cot["g_scale"].double()
    loss = (dxyz * g).sum() + (drot * h).sum() + (dsc * s).sum() + 0.0 * rho.sum()
    names = {"g_trans": tr, "g_rot": ro, "g_scale": sc, "g_local_rot": lq, "g_radius": rho, "g_weight": wl, "g_nodes_hyper": nh,
             "g_feature": fh, "g_mask": m}
    leaves = {k: t_ for k, t_ in names.items() if t_ is not None}
    grads = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)))
    ref = {k: (torch.zeros_like(leaves[k]) if gr is None else gr).detach() for k, gr in grads.items()}
    with torch.no_grad():
        ag, ah, as_ = g.abs(), h.abs(), s.abs()
        md = mm.detach()
        yd, roi, sci = y.detach(), roe.detach()[idx], sc.detach()[idx]
        A = am * ((ag[:, None] * Ay).sum(-1) + (ah[:, None] * Aro).sum(-1) + (as_[:, None] * Asc).sum(-1))
        a = md * ((g[:, None] * yd).sum(-1) + (h[:, None] * roi).sum(-1) + (s[:, None] * sci).sum(-1))
        da = am * ((ag[:, None] * dy).sum(-1) + (ah[:, None] * dro).sum(-1)) + 14 * U * A
        wa = (wd * a).sum(1, keepdim=True)
        dwa = (dw * A + wd * da).sum(1, keepdim=True) + (K + 1) * U * (wd * A).sum(1, keepdim=True)
        num = a - wa
        c = num / Sd
        dc = (da + dwa + U * (a.abs() + wa.abs())) / Sd + num.abs() / Sd * (dS / Sd + 2 * U)
        ac = c.abs()
        cnt = torch.bincount(flat, minlength=M)
        LU = (depth_reduce(cnt).double() * U)

        def node(term, err):
            extra = (1,) * (term.dim() - 2)
            return _scat(M, flat, err + TINY * (term != 0)) + LU.reshape((M,) + extra) * _scat(M, flat, term.abs())

        c1, dc1 = wd * md, am * (dw + 2 * U * wd)
        for key, cotv, acot in (("g_trans", g, ag), ("g_rot", h, ah), ("g_scale", s, as_)):
            res[key] = (ref[key], node(c1[..., None] * cotv[:, None], dc1[..., None] * acot[:, None]))
        if local_frame:
            TR = (c1[..., None, None] * g[:, None, :, None] * rel[:, :, None, :]).reshape(N, K, 9)
            eR = ((dc1 + 2 * U * wd * am)[..., None, None] * ag[:, None, :, None] * arel[:, :, None, :]).reshape(N, K, 9)
            G, bG = _scat(M, flat, TR), node(TR, eR)
            q = lq.detach() + E
            res["g_local_rot"] = (ref["g_local_rot"], _dq_abs(q, bG) + 16 * U * _dq_abs(q, G.abs() + bG))
        q19 = ud * dd_ / r2d
        res["g_radius"] = (ref["g_radius"], node(c * q19, dc * q19 + ac * (du * dd_ / r2d + q19 * (DIST_W + R2_REL + 3 * U))))
        if wl is not None:
            Tw = c * ed
            Sw, bS = _scat(M, flat, Tw), node(Tw, dc * ed + ac * (de + U * ed))
            sg = torch.sigmoid(wl.detach())
            ds1 = sg * SIG_REL + U * (1 - sg)
            res["g_weight"] = (ref["g_weight"], bS * sg * (1 - sg) + Sw.abs() * (sg * SIG_REL * (1 - sg) + sg * ds1)
                               + 2 * U * ref["g_weight"].abs())
        if hyper:
            dfd = diff.detach()
            Th = (c * ud / r2d)[..., None] * dfd
            eh = dfd.abs() * ((dc * ud + ac * du + ac * ud * (R2_REL + 6 * U)) / r2d)[..., None] + TINY * (Th != 0)
            res["g_nodes_hyper"] = (ref["g_nodes_hyper"], node(Th, eh))
            res["g_feature"] = (ref["g_feature"], eh.sum(1) + K * U * Th.abs().sum(1))
        if m is not None:
            mag = (ag * (wAy + (x64.abs() if local_frame else 0.0))).sum(1) + (ah * (wAro + bias * E)).sum(1) + (as_ * wAsc).sum(1)
            res["g_mask"] = (ref["g_mask"], (ag * dts).sum(1) + (ah * drs).sum(1) + (as_ * dss).sum(1) + 12 * U * mag)
    return res
